"""GPU TIFF strip deflate (vcf_zlib_strips, csrc/vcf_deflate.hip) against
zlib.compress, byte for byte, and the TIFF files around the strips against the
host writer (the reference's TIFF.py:29 via tifffile -> zlib level 6)."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _frames(n, shape, seed, kind="image"):
    rng = np.random.default_rng(seed)
    out = []
    for f in range(n):
        if kind == "image":
            H, W, C = shape
            y = np.arange(H)[:, None, None]
            x = np.arange(W)[None, :, None]
            a = 128 + 60 * np.sin(x / (37 + f) + np.arange(C)) + 50 * np.cos(y / 23.0 - f) + rng.normal(0, 4, shape)
            out.append(np.clip(a, 0, 255).astype(np.uint8))
        elif kind == "random":
            out.append(rng.integers(0, 256, shape, dtype=np.uint8))
        else:   # DCT-index-like: mostly 128 with sparse values
            a = np.full(shape, 128, np.uint8)
            m = rng.random(shape) < 0.03
            a[m] = rng.integers(100, 160, int(m.sum()))
            out.append(a)
    return np.stack(out)


def _check(frames, strip_bytes, level=6):
    from vcf_amd.device import DeviceBuffer
    from vcf_amd.zlib_gpu import StripDeflater
    n = frames.shape[0]
    flat = frames.reshape(n, -1)
    d = DeviceBuffer.from_array(flat)
    got = StripDeflater().deflate_device(d, n, flat.shape[1], strip_bytes, level)
    for f in range(n):
        b = flat[f].tobytes()
        want = [zlib.compress(b[i:i + strip_bytes], level) for i in range(0, len(b), strip_bytes)]
        assert len(got[f]) == len(want)
        for k, (g, w) in enumerate(zip(got[f], want)):
            assert g == w, (f, k, len(g), len(w))


@pytest.mark.parametrize("kind", ["image", "random", "sparse"])
def test_strips_equal_zlib(kind):
    _check(_frames(3, (40, 300, 3), 1, kind), 11 * 900)


@pytest.mark.parametrize("strip", [65536, 65300, 65280, 65274, 1, 2, 3, 258, 4096])
def test_strip_lengths(strip):
    _check(_frames(2, (48, 700, 3), 2, "image"), strip)


def test_slide_nil_head():
    """zlib's slide_hash maps the head entry at input position wsize to NIL
    (tests/deflate_cases.py): the GPU must emit zlib's literal there."""
    from deflate_cases import slide_nil_strip
    from vcf_amd.device import DeviceBuffer
    from vcf_amd.zlib_gpu import StripDeflater
    b = np.frombuffer(slide_nil_strip(), np.uint8)
    frames = np.stack([b, b[::-1].copy()])
    d = DeviceBuffer.from_array(frames)
    for level in (4, 6, 9):
        got = StripDeflater().deflate_device(d, 2, b.size, b.size, level)
        assert got[0][0] == zlib.compress(b.tobytes(), level), level
        assert got[1][0] == zlib.compress(b[::-1].tobytes(), level), level


@pytest.mark.parametrize("level", [4, 5, 7, 8, 9])
def test_levels(level):
    _check(_frames(1, (30, 1000, 3), 3, "image"), 65536, level)


def test_1080p_dct_frame_equals_host_tiff():
    """A 1080p frame of DCT indices (the C2 path): the GPU TIFF equals the host writer's bytes."""
    from vcf_amd.synthetic import synth_frame
    from vcf_amd.codec.tiff import imwrite_bytes
    from vcf_amd.device import DeviceBuffer
    from vcf_amd.zlib_gpu import tiff_frames_device
    from vcf_amd import dct
    rgb = np.stack([synth_frame(1080, 1920, s) for s in (1, 2)])
    k = dct.encode(rgb, Q=32)
    d = DeviceBuffer.from_array(np.ascontiguousarray(k))
    files = tiff_frames_device(d, 2, k.shape[1:], np.uint8)
    for f in range(2):
        assert files[f] == imwrite_bytes(k[f])


def test_u16_and_gray():
    from vcf_amd.codec.tiff import imwrite_bytes
    from vcf_amd.device import DeviceBuffer
    from vcf_amd.zlib_gpu import tiff_frames_device
    rng = np.random.default_rng(5)
    a = (rng.integers(0, 600, (3, 70, 130, 3))).astype(np.uint16)
    files = tiff_frames_device(DeviceBuffer.from_array(a), 3, a.shape[1:], np.uint16)
    assert all(files[f] == imwrite_bytes(a[f]) for f in range(3))
    g = rng.integers(120, 136, (2, 300, 333), dtype=np.uint8)
    files = tiff_frames_device(DeviceBuffer.from_array(g), 2, g.shape[1:], np.uint8)
    assert all(files[f] == imwrite_bytes(g[f]) for f in range(2))


def test_unsupported():
    from vcf_amd import _lib as L
    from vcf_amd.device import DeviceBuffer
    d = DeviceBuffer(1 << 20)
    for level, strip in ((1, 4096), (6, 65537), (0, 4096)):
        with pytest.raises(Exception):
            L.call("vcf_zlib_strips", d.ptr, 1, 8192, strip, level, d.ptr, 1 << 17, d.ptr, d.ptr, None)


def test_device_iii_tiff_equals_host_writer():
    """The C4 data path with the reference's default -c TIFF
    (vcf_amd/codec/iii_device.py, entropy="TIFF"): every gathered file equals
    the host TIFF writer's (system zlib) for the frame's indices, and reads back."""
    from vcf_amd.codec.iii_device import DeviceIII
    from vcf_amd.codec.tiff import imread_bytes, imwrite_bytes
    from vcf_amd import dct
    from vcf_amd.device import DeviceBuffer
    rng = np.random.default_rng(3)
    for n, H, W in ((5, 61, 77), (3, 200, 1000)):
        y = np.arange(H)[:, None, None]
        x = np.arange(W)[None, :, None]
        frames = np.stack([np.clip(128 + 50 * np.sin(x / (19 + f) + y / 31.0 + np.arange(3)) +
                                   rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8) for f in range(n)])
        job = DeviceIII(None, 0, 1, n, H, W, 32, entropy="TIFF")
        stages = {}
        sizes, got = job.run(DeviceBuffer.from_array(frames), stages)
        k = dct.encode(frames, Q=32)
        for i in range(n):
            want = imwrite_bytes(k[i])
            assert got[i] == want and sizes[i] == len(want), (n, i)
            assert np.array_equal(imread_bytes(bytes(got[i])), k[i])


def _golden_tif_cases():
    import glob
    import os
    from conftest import GOLDEN
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "dct_*.npz")))


@pytest.mark.parametrize("name", _golden_tif_cases())
def test_gpu_tiff_equals_reference_files(name):
    """The GPU deflate pinned to the reference's own bytes: the
    TIFF of every golden case's index array `k`, deflated on the GPU
    (tiff_frames_device), equals the .tif the reference's 2D-DCT.py wrote
    (tests/golden/dct_*.npz 'tif', tifffile 2021.7.2 + zlib, make_golden*.py)."""
    import os
    from conftest import GOLDEN
    from vcf_amd.device import DeviceBuffer
    from vcf_amd.zlib_gpu import covers, tiff_frames_device
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    k = np.ascontiguousarray(z["k"])
    if k.dtype not in (np.uint8, np.uint16) or not covers(k.shape, k.dtype.itemsize):
        pytest.skip(f"{k.dtype} {k.shape}: not a TIFF the GPU deflate covers")
    files = tiff_frames_device(DeviceBuffer.from_array(k), 1, k.shape, k.dtype)
    assert files[0] == z["tif"].tobytes()


@pytest.mark.parametrize("name", ["smooth_512x512", "rand_512x512"])
def test_gpu_tiff_512_matches_reference_sha256(manifest, name):
    """The C1 cases by SHA-256 (tests/golden/manifest.json big_cases): the GPU
    deflate of the indices gives the reference's .tif."""
    import hashlib
    import importlib.util
    import os
    from conftest import GOLDEN
    from vcf_amd import dct
    from vcf_amd.device import DeviceBuffer
    from vcf_amd.zlib_gpu import tiff_frames_device
    case = [c for c in manifest["big_cases"] if c["name"] == name][0]
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    rgb = m.synth(case["kind"], case["H"], case["W"], case["seed"])
    k = dct.encode(rgb, Q=32)
    tif = tiff_frames_device(DeviceBuffer.from_array(np.ascontiguousarray(k)), 1, k.shape, np.uint8)[0]
    assert len(tif) == case["encode_bytes"]
    assert hashlib.sha256(tif).hexdigest() == case["sha256"]["tif"]


def test_c4_workload_every_strip_equals_zlib():
    """bench.py's C4 content (256 1080p DCT index frames, 25 344 strips): several
    workspace rounds, lazy and register-window strips side by side.  Every strip
    against zlib.compress: a strip coded from stale workspace data (the previous
    round's strip in the same slot) shows up here."""
    from concurrent.futures import ThreadPoolExecutor

    from vcf_amd import synthetic as bench
    from vcf_amd import dct
    from vcf_amd.codec.tiff import strip_layout
    from vcf_amd.device import DeviceBuffer
    from vcf_amd.zlib_gpu import StripDeflater
    n, H, W = 256, 1080, 1920
    bases = [bench.synth_frame(H, W, seed=100 + s) for s in range(4)]
    k = np.concatenate([dct.encode(np.stack([bench.c4_frame(bases, i) for i in range(f, f + 16)]), Q=32)
                        for f in range(0, n, 16)])
    flat = np.ascontiguousarray(k.reshape(n, -1))
    sb = strip_layout(k.shape[1:], 1)[2]
    got = StripDeflater().deflate_device(DeviceBuffer.from_array(flat), n, flat.shape[1], sb, 6)
    spf = len(got[0])
    with ThreadPoolExecutor(16) as ex:
        want = list(ex.map(lambda s: zlib.compress(flat[s // spf, (s % spf) * sb:(s % spf + 1) * sb].tobytes(), 6),
                           range(n * spf)))
    bad = [s for s in range(n * spf) if bytes(got[s // spf][s % spf]) != want[s]]
    assert not bad, bad[:20]


_MULTI_ROUND = r'''
import sys, zlib
import numpy as np
sys.path.insert(0, sys.argv[1])
from vcf_amd import synthetic as bench
from vcf_amd import dct
from vcf_amd import _lib as L
from vcf_amd.codec.tiff import strip_layout
from vcf_amd.device import DeviceBuffer
from vcf_amd.zlib_gpu import StripDeflater
L.call("vcf_zlib_set_workspace_budget", int(sys.argv[2]))
n, H, W = 24, 1080, 1920
bases = [bench.synth_frame(H, W, seed=100 + s) for s in range(4)]
k = np.concatenate([dct.encode(np.stack([bench.c4_frame(bases, i) for i in range(f, f + 8)]), Q=32)
                    for f in range(0, n, 8)])
flat = np.ascontiguousarray(k.reshape(n, -1))
sb = strip_layout(k.shape[1:], 1)[2]
total = n * int(L.lib().vcf_zlib_strip_count(flat.shape[1], sb))
per = int(L.lib().vcf_zlib_workspace(total)) // (int(L.lib().vcf_zlib_workspace(1)))
got = StripDeflater().deflate_device(DeviceBuffer.from_array(flat), n, flat.shape[1], sb, 6)
spf = len(got[0])
bad = [s for s in range(n * spf)
       if bytes(got[s // spf][s % spf]) != zlib.compress(flat[s // spf, (s % spf) * sb:(s % spf + 1) * sb].tobytes(), 6)]
print("strips", total, "per_round", per, "bad", len(bad))
assert per < total and not bad, bad[:20]
'''


def test_many_rounds_every_strip_equals_zlib():
    """Deterministic multi-round run: the workspace budget forced down to ~50 MB
    (vcf_zlib_set_workspace_budget, per-process state, so a child process) cuts 2 376 C4
    strips into rounds of 43 that reuse one workspace; every strip against
    zlib.compress (a strip coded from the previous round's tables shows here)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _MULTI_ROUND, root, "50000000"], capture_output=True, text=True,
                       timeout=280)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "bad 0" in p.stdout


# ---- the named corpus (tests/deflate_cases.py): both parse paths in one call ----
# tests/test_deflate.py asserts what the corpus holds (lazy and non-lazy strips,
# multi-block strips, matches past the lazy parse's LDS window, at MAX_DIST, ...)
# and that the host restatement of the algorithm codes every entry as zlib does.
_state = {}


def _deflater():
    """One deflater for the corpus tests: its scratch (and the LDS its kernels
    leave behind) carries over from one call to the next, as in the product."""
    from vcf_amd.zlib_gpu import StripDeflater
    if "deflater" not in _state:
        _state["deflater"] = StripDeflater()
    return _state["deflater"]


def _want(b: bytes, level: int) -> bytes:
    """zlib.compress, computed once per (strip, level) for the whole module."""
    cache = _state.setdefault("want", {})
    key = (b, level)
    if key not in cache:
        cache[key] = zlib.compress(b, level)
    return cache[key]


def _deflate(frame_list, strip_bytes, level, offset=0):
    """Every strip of equal-length frames (bytes) through one call -> flat list of
    (label suffix, strip bytes, stream)."""
    from vcf_amd.device import DeviceBuffer
    fb = len(frame_list[0])
    assert all(len(f) == fb for f in frame_list)
    host = np.zeros(offset + fb * len(frame_list), np.uint8)
    host[offset:] = np.frombuffer(b"".join(frame_list), np.uint8)
    d = DeviceBuffer.from_array(host)
    got = _deflater().deflate_device(d, len(frame_list), fb, strip_bytes, level, offset=offset)
    d.free()
    out = []
    for f, b in enumerate(frame_list):
        strips = [b[i:i + strip_bytes] for i in range(0, fb, strip_bytes)]
        assert len(got[f]) == len(strips)
        out += [((f, k), s, bytes(g)) for k, (s, g) in enumerate(zip(strips, got[f]))]
    return out


def _assert_zlib(result, level, label):
    """Every strip of a _deflate result equals zlib.compress; the failure names the
    strips and the first differing token of the first one."""
    from deflate_cases import describe_mismatch
    bad = [(label(fk), s, g) for fk, s, g in result if g != _want(s, level)]
    if bad:
        name, s, g = bad[0]
        raise AssertionError(f"level {level}: {len(bad)} of {len(result)} strips differ from zlib: "
                             f"{[b[0] for b in bad[:12]]}; first ({name}, {len(s)} bytes): "
                             f"{describe_mismatch(g, _want(s, level))}")


def _corpus_call(length, level):
    """The corpus entries of one length as the frames of one call (one strip each)."""
    from deflate_cases import corpus_by_length
    entries = corpus_by_length()[length]
    res = _deflate([b for _, b in entries], length, level)
    return entries, res


@pytest.mark.parametrize("level", [6, 9, 4, 5, 7, 8])
def test_corpus_equals_zlib(level):
    """Every corpus entry at this level: the 64 KiB entries (19 lazy, 11 non-lazy
    by K1's rule) side by side in one call, the other lengths in a call each."""
    from deflate_cases import corpus, corpus_by_length
    seen = 0
    for length in corpus_by_length():
        entries, res = _corpus_call(length, level)
        _assert_zlib(res, level, lambda fk: entries[fk[0]][0])
        seen += len(res)
    assert seen == len(corpus())


def _assert_parse_info(strips, labels, want_listed=None):
    """The kernel's parse order and distinct count of the last call against
    lazy_rule's; -> (lazy strips, non-lazy strips)."""
    from deflate_cases import lazy_rule
    info = _deflater().parse_info()
    rule = [lazy_rule(s) for s in strips]
    bad = [(labels[i], rule[i], int(info["distinct"][i]), bool(info["lazy"][i])) for i in range(len(strips))
           if rule[i][0] != info["distinct"][i] or rule[i][2] != info["lazy"][i]]
    assert not bad, bad[:10]
    n_lazy = sum(r[2] for r in rule)
    assert info["listed"] == len(strips) - n_lazy, (info["listed"], len(strips), n_lazy)
    return n_lazy, len(strips) - n_lazy


def test_corpus_takes_the_path_it_was_written_for():
    """K1's parse order word and distinct count of every strip (read back from the
    workspace, StripDeflater.parse_info) equal the host rule the corpus properties
    are asserted with, and K1's list of non-lazy strips has their number: the
    64 KiB call runs at least 10 strips through each parse."""
    from deflate_cases import STRIP, corpus_by_length
    for length in corpus_by_length():
        entries, res = _corpus_call(length, 6)
        n_lazy, n_non = _assert_parse_info([s for _, s, _ in res], [e[0] for e in entries])
        print(f"length {length}: {n_lazy} lazy, {n_non} non-lazy")
        if length == STRIP:
            assert n_lazy >= 10 and n_non >= 10, (n_lazy, n_non)


@pytest.mark.parametrize("tail", [1, 2, 3])
def test_long_side_lists(tail):
    """More than 4 096 non-lazy strips in one round: the side kernels' grids
    (256 / 128 / 4 096 workgroups) wrap around K1's list, with 320 lazy strips
    interleaved and a last strip of 1, 2 or 3 bytes."""
    from deflate_cases import small_strip_frame
    frame = small_strip_frame(272, 4500, 320, tail)
    res = _deflate([frame], 272, 6)
    assert len(res) == 4821 and len(res[-1][1]) == tail
    _assert_zlib(res, 6, lambda fk: f"strip {fk[1]}")
    n_lazy, n_non = _assert_parse_info([s for _, s, _ in res], list(range(len(res))))
    print(f"tail {tail}: {n_lazy} lazy, {n_non} non-lazy (K1's list)")
    assert n_non > 4096 and n_lazy >= 300, (n_lazy, n_non)


@pytest.mark.parametrize("level", [6, 9, 4])
def test_side_list_of_two_chunk_strips(level):
    """300 non-lazy strips of 5 000 bytes (two K2a chunks each, a K2b worklist split
    over 4 workgroups) on grids of 256 / 128, 60 lazy strips interleaved."""
    from deflate_cases import small_strip_frame
    res = _deflate([small_strip_frame(5000, 300, 60)], 5000, level)
    _assert_zlib(res, level, lambda fk: f"strip {fk[1]}")
    n_lazy, n_non = _assert_parse_info([s for _, s, _ in res], list(range(len(res))))
    assert n_non >= 290 and n_lazy >= 50, (n_lazy, n_non)


_ROUNDS = r'''
import sys, zlib
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from deflate_cases import STRIP, corpus_by_length, describe_mismatch, lazy_rule, small_strip_frame
from vcf_amd.device import DeviceBuffer
from vcf_amd import _lib as L
from vcf_amd.zlib_gpu import StripDeflater, workspace
L.call("vcf_zlib_set_workspace_budget", int(sys.argv[3]))
calls = [("corpus", [b for _, b in corpus_by_length()[STRIP]], STRIP),
         ("5000", [small_strip_frame(5000, 300, 60)], 5000)]
dfl = StripDeflater()
for what, frames, sb in calls:
    strips = [f[i:i + sb] for f in frames for i in range(0, len(f), sb)]
    per = workspace(len(strips)) // workspace(1)
    rounds = -(-len(strips) // per)
    n_lazy = sum(lazy_rule(s)[2] for s in strips)
    d = DeviceBuffer.from_array(np.frombuffer(b"".join(frames), np.uint8))
    got = [g for f in dfl.deflate_device(d, len(frames), len(frames[0]), sb, 6) for g in f]
    bad = [i for i, (g, s) in enumerate(zip(got, strips)) if bytes(g) != zlib.compress(s, 6)]
    print(what, "strips", len(strips), "lazy", n_lazy, "per_round", per, "rounds", rounds, "bad", bad[:20])
    if bad:
        print(describe_mismatch(got[bad[0]], zlib.compress(strips[bad[0]], 6)))
    assert rounds > 1 and len(got) == len(strips) and not bad
    assert 0 < n_lazy < len(strips)
print("all rounds ok")
'''


@pytest.mark.parametrize("per_round", [6, 1])
def test_rounds_with_both_kinds(per_round):
    """The 64 KiB corpus call and the 5 000-byte call in rounds of 6 strips and of
    one strip (vcf_zlib_set_workspace_budget, per-process state: a child process): K1's list
    is reset every round and the side kernels read the list of this round's slots."""
    import os
    import subprocess
    import sys
    from vcf_amd.zlib_gpu import workspace
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    budget = per_round * workspace(1) + (4096 if per_round > 1 else 0)
    p = subprocess.run([sys.executable, "-c", _ROUNDS, root, os.path.join(root, "tests"), str(budget)],
                       capture_output=True, text=True, timeout=120)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "all rounds ok" in p.stdout and f"per_round {per_round} " in p.stdout


@pytest.mark.parametrize("strip", [4099, 65521])
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_unaligned_source(offset, strip):
    """Frames from an odd byte offset, odd strip lengths: over two frames of three
    strips the strip starts take every residue mod 4 (K1's dword staging, K2's
    window fill, the lazy parse's window fill and far compares); lazy
    (sparse_rows_7873) and non-lazy (skewed) content."""
    from deflate_cases import corpus
    c = corpus()
    frames = [np.resize(np.frombuffer(c[name], np.uint8), 3 * strip).tobytes()
              for name in ("sparse_rows_7873", "skewed")]
    names = ["sparse_rows_7873", "skewed"]
    for level in (6, 9):
        res = _deflate(frames, strip, level, offset=offset)
        assert len(res) == 6
        _assert_zlib(res, level, lambda fk: f"{names[fk[0]]} strip {fk[1]} offset {offset}")
    n_lazy, n_non = _assert_parse_info([s for _, s, _ in res], [f"{names[i // 3]} {i % 3}" for i in range(6)])
    assert n_lazy == 3 and n_non == 3


def test_corpus_three_runs_identical():
    """The level-6 corpus call three times in one process with another deflate (the
    long-list call) in between: the same bytes every time, whatever the other
    call's workgroups left in LDS and in the workspace."""
    from deflate_cases import STRIP, small_strip_frame
    runs = []
    for r in range(3):
        entries, res = _corpus_call(STRIP, 6)
        runs.append([g for _, _, g in res])
        if r == 0:
            _assert_zlib(res, 6, lambda fk: entries[fk[0]][0])
        if r < 2:
            _deflate([small_strip_frame(272, 4500, 320, 1)], 272, 6)
    for r in (1, 2):
        diff = [entries[i][0] for i in range(len(entries)) if runs[r][i] != runs[0][i]]
        assert not diff, (r, diff)

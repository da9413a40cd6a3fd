"""The coded motion field without a GPU: the host coder (vcf_amd/csrc/vcf_mvc.cpp)
against the plain-Python restatement of the rule (tests/mvc_ref.py), corrupt
streams, the .vmv container (vcf_amd/codec/mvfile.py), the properties of the
restated refinement, and --mvc / --mv_lambda through the IPP codec over numpy
tools."""
import ctypes
import json
import struct
import types

import numpy as np
import pytest

import mvc_ref as M
import subpel_ref as R
import test_obmc as T

import vcf_amd._lib as L
from vcf_amd import ipp as K
from vcf_amd.codec import mvfile

FIELDS = [(1, 1), (1, 7), (5, 1), (6, 9)]


def _field(rng, shape, step, extremes=True):
    q = (rng.integers(-400, 401, shape + (2,)) * step).astype(np.int32)
    if extremes:                      # vectors of +-2^15 next to small ones
        flat = q.reshape(-1)
        flat[0], flat[-1] = 1 << 15, -(1 << 15)
        flat[flat.size // 2] = -(1 << 15)
    return q


@pytest.mark.parametrize("shape", FIELDS)
@pytest.mark.parametrize("step", [1, 2, 4])
def test_encoder_equals_the_rule_and_the_decoder_inverts_it(shape, step):
    rng = np.random.Generator(np.random.PCG64(100 * shape[0] + 10 * shape[1] + step))
    for extremes in (False, True):
        q = _field(rng, shape, step, extremes)
        s = K.mv_encode(q, step)
        assert s == M.encode(q, step)
        assert np.array_equal(K.mv_decode(s, *shape, step), q)
        assert np.array_equal(M.decode(s, *shape, step), q)
    z = np.zeros(shape + (2,), np.int32)
    s = K.mv_encode(z, step)
    n = 2 * shape[0] * shape[1]                                  # one "1" per component, then zero padding
    assert s == M.encode(z, step) and len(s) == (n + 7) // 8
    assert int.from_bytes(s, "big") == ((1 << n) - 1) << (-n % 8)
    assert np.array_equal(K.mv_decode(s, *shape, step), z)


def test_empty_fields():
    for shape in ((0, 5), (3, 0)):
        assert K.mv_encode(np.zeros(shape + (2,), np.int32), 2) == b""
        assert K.mv_decode(b"", *shape, 2).shape == shape + (2,)
        with pytest.raises(ValueError):
            K.mv_decode(b"\0", *shape, 2)


def test_code_length_equals_the_written_code():
    """len(d) against the code as written: the restatement's for |d| <= 70 000, and the library's for
    every d it can reach, |d| <= 2^16: a first row (p = the left vector) that swings between -2^15
    and -2^15 + d codes +d and -d in turn, and the library's bytes equal the restatement's."""
    for d in range(-70000, 70001):
        assert M.length(d) == len(M.code_bits(d))
    for d, n in ((0, 1), (1, 3), (-1, 3), (2, 5), (-3, 5), (4, 7), (65536, 35), (-65536, 35)):
        assert M.length(d) == n
    lo = -(1 << 15)
    for axis in (0, 1):
        for ds in (range(1, 1 << 16, 7), range((1 << 16) - 300, (1 << 16) + 1)):
            ds = list(ds)
            q = np.zeros((1, 2 * len(ds) + 1, 2), np.int32)
            q[0, :, axis] = lo
            q[0, 1::2, axis] += ds
            s = K.mv_encode(q, 1)
            assert s == M.encode(q, 1)
            bits = M.length(lo) + 2 * sum(M.length(d) for d in ds) + q.shape[1]   # the other component: 1 bit each
            assert len(s) == (bits + 7) // 8
            assert np.array_equal(K.mv_decode(s, 1, q.shape[1], 1), q)


def _raw_decode(data, nby, nbx, step):
    buf = np.frombuffer(bytes(data) + b"\xff" * 8, np.uint8)     # set bits past the stream: never to be read
    q = np.zeros((nby, nbx, 2), np.int32)
    return L.lib().vcf_mv_decode(buf.ctypes.data, len(data), nby, nbx, step, q.ctypes.data)


def _rejected(data, nby, nbx, step):
    assert _raw_decode(data, nby, nbx, step) == L.VCF_ERR_INVALID
    assert L.lib().vcf_last_error()
    with pytest.raises(ValueError):
        K.mv_decode(data, nby, nbx, step)
    with pytest.raises(ValueError):
        M.decode(data, nby, nbx, step)


def _bits(s):
    s += "0" * (-len(s) % 8)
    return bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8))


def test_corrupt_streams_are_rejected_with_a_status():
    rng = np.random.Generator(np.random.PCG64(5))
    q = _field(rng, (6, 9), 1)
    s = K.mv_encode(q, 1)
    assert _raw_decode(s, 6, 9, 1) == L.VCF_OK
    for n in range(len(s)):                                   # every truncation
        _rejected(s[:n], 6, 9, 1)
    _rejected(s + b"\0", 6, 9, 1)                             # bytes after the last code
    # padding: a stream of 2 * 3 one-bit codes leaves two padding bits
    z = K.mv_encode(np.zeros((1, 3, 2), np.int32), 1)
    assert z == b"\xfc"
    for flip in (1, 2, 3):
        _rejected(bytes([z[0] | flip]), 1, 3, 1)
    # a prefix of 17 zeros is the longest legal one (d = -2^16 from p = 2^15 is out of range, d = 2^16 from
    # -2^15 is not); 18 zeros are rejected however the code goes on
    ok = np.array([[[-(1 << 15), 0], [1 << 15, 0]]], np.int32)
    assert _raw_decode(K.mv_encode(ok, 1), 1, 2, 1) == L.VCF_OK
    for tail in ("1" + "0" * 18, "1" * 19, ""):
        _rejected(_bits("0" * 18 + tail + "1" * 8), 1, 1, 1)
    # an overflowing vector: d = 2^15 + 1 from p = 0, and d = 1 at step 4 from p = 2^15
    _rejected(_bits(M.code_bits((1 << 15) + 1) + "1"), 1, 1, 1)
    _rejected(_bits(M.code_bits(-(1 << 15) - 1) + "1"), 1, 1, 1)
    _rejected(_bits("1" + M.code_bits(1 << 16)), 1, 1, 1)
    _rejected(_bits(M.code_bits(1 << 13) + "1" + M.code_bits(1) + "1"), 1, 2, 4)
    for step in (0, 3, 8, -1):
        assert _raw_decode(s, 6, 9, step) == L.VCF_ERR_INVALID
        with pytest.raises(ValueError):
            K.mv_decode(s, 6, 9, step)
        with pytest.raises(ValueError):
            K.mv_encode(q, step)
    assert L.lib().vcf_mv_decode(None, 0, 1, 1, 1, q.ctypes.data) == L.VCF_ERR_INVALID
    assert L.lib().vcf_mv_decode(q.ctypes.data, 4, 1, 1, 1, None) == L.VCF_ERR_INVALID
    assert L.lib().vcf_mv_decode(q.ctypes.data, 4, -1, 9, 1, q.ctypes.data) == L.VCF_ERR_INVALID


def test_encoder_argument_errors():
    lib = L.lib()
    rng = np.random.Generator(np.random.PCG64(6))
    q = _field(rng, (6, 9), 2)
    want = M.encode(q, 2)
    n = ctypes.c_int64(-1)
    cap = ctypes.c_int64(0)
    assert lib.vcf_mv_encode_bound(6, 9, ctypes.byref(cap)) == L.VCF_OK and cap.value >= len(want)
    assert lib.vcf_mv_encode_bound(6, 9, None) == L.VCF_ERR_INVALID
    assert lib.vcf_mv_encode_bound(-1, 9, ctypes.byref(cap)) == L.VCF_ERR_INVALID
    guard = 16
    for c in (len(want), len(want) - 1, len(want) // 2, 1, 0, -1):          # a too small cap: nothing past it is written
        out = np.full(len(want) + guard, 0xA5, np.uint8)
        rc = lib.vcf_mv_encode(q.ctypes.data, 6, 9, 2, out.ctypes.data, c, ctypes.byref(n))
        assert rc == (L.VCF_OK if c == len(want) else L.VCF_ERR_INVALID), c
        assert np.all(out[max(c, 0):] == 0xA5), c
        if rc == L.VCF_OK:
            assert n.value == len(want) and out[:c].tobytes() == want
    out = np.zeros(cap.value, np.uint8)
    for bad in (q + 1, q * 0 + 3):                                           # off the step grid
        bad = np.ascontiguousarray(bad, np.int32)
        assert lib.vcf_mv_encode(bad.ctypes.data, 6, 9, 2, out.ctypes.data, cap.value, ctypes.byref(n)) == L.VCF_ERR_INVALID
        with pytest.raises(ValueError):
            M.encode(bad, 2)
    for v in ((1 << 15) + 4, -(1 << 15) - 4, 1 << 30):                       # beyond +-2^15
        big = q.copy()
        big[3, 4, 1] = v
        assert lib.vcf_mv_encode(big.ctypes.data, 6, 9, 2, out.ctypes.data, cap.value, ctypes.byref(n)) == L.VCF_ERR_INVALID
        with pytest.raises(ValueError):
            K.mv_encode(big, 2)
    for args in ((None, 6, 9, 2, out.ctypes.data, cap.value, ctypes.byref(n)),
                 (q.ctypes.data, 6, 9, 2, None, cap.value, ctypes.byref(n)),
                 (q.ctypes.data, 6, 9, 2, out.ctypes.data, cap.value, None)):
        assert lib.vcf_mv_encode(*args) == L.VCF_ERR_INVALID


# ---- the container ----------------------------------------------------------------------------

def _motion(rng, n_p, n_b, nby, nbx, subpel):
    step = 4 // subpel
    f = lambda *shape: (rng.integers(-60, 61, shape + (nby, nbx, 2)) * step / 4.0).astype(np.float32)
    return f(n_p), (f(n_b, 2) if n_b else None)


@pytest.mark.parametrize("subpel", [1, 2, 4])
def test_container_round_trip(tmp_path, subpel):
    rng = np.random.Generator(np.random.PCG64(subpel))
    nby, nbx = 6, 8
    for n_p, n_b, kind in ((3, 0, None), (3, 0, "R"), (2, 3, "B"), (0, 0, None)):
        mv, bmv = _motion(rng, n_p, n_b, nby, nbx, subpel)
        modes = None if kind is None else rng.integers(0, 3 if kind == "B" else 2, ((n_b if kind == "B" else n_p), nby, nbx),
                                                       dtype=np.uint8)
        path = str(tmp_path / f"m{n_p}{n_b}{kind}.vmv")
        n = mvfile.write(path, mv, subpel, bmv=bmv, modes=modes)
        data = open(path, "rb").read()
        assert n == len(data) and data[:4] == b"VMV1"
        assert struct.unpack_from("<6I", data, 4) == (nby, nbx, subpel, n_p, n_b, int(modes is not None))
        # the first field's payload is the coder's
        if n_p:
            ln, = struct.unpack_from("<I", data, 28)
            assert data[32:32 + ln] == M.encode(np.rint(mv[0] * 4).astype(np.int64), 4 // subpel)
        f = mvfile.read(path)
        assert np.array_equal(f["mv_f32"], mv) and f["mv_f32"].dtype == np.float32
        assert (f["bmv_f32"] is None) if bmv is None else np.array_equal(f["bmv_f32"], bmv)
        assert (f["modes"] is None) if modes is None else np.array_equal(f["modes"], modes)
        mvfile.check_header(f, nby, nbx, subpel, n_p, n_b)
        for k, v in (("nby", nby + 1), ("nbx", nbx - 1), ("subpel", 3 - subpel if subpel < 4 else 2), ("n_P", n_p + 1),
                     ("n_B", n_b + 1)):
            want = dict(nby=nby, nbx=nbx, subpel=subpel, n_P=n_p, n_B=n_b)
            want[k] = v
            with pytest.raises(ValueError, match="header disagrees"):
                mvfile.check_header(f, want["nby"], want["nbx"], want["subpel"], want["n_P"], want["n_B"])
        with pytest.raises(ValueError, match="after the last stream"):
            mvfile.unpack(data + b"\0")
        for cut in range(0, len(data), 5):
            with pytest.raises(ValueError):
                mvfile.unpack(data[:cut])


def test_container_rejects_what_it_does_not_write():
    rng = np.random.Generator(np.random.PCG64(9))
    mv, bmv = _motion(rng, 2, 1, 3, 4, 4)
    modes = rng.integers(0, 3, (1, 3, 4), dtype=np.uint8)
    data = bytearray(mvfile.pack(mv, 4, bmv=bmv, modes=modes))
    mvfile.unpack(bytes(data))
    # (another legal subpel may still parse: that is check_header's to catch, against meta.json)

    def with_u32(off, v):
        d = bytearray(data)
        struct.pack_into("<I", d, off, v)
        return bytes(d)
    for off, v in ((0, 0x31564d57), (4, 4), (4, 1 << 30), (8, 5), (12, 3), (16, 3), (16, 1 << 31), (20, 0), (20, 2),
                   (24, 0), (24, 2), (28, 0), (28, 1 << 20)):
        with pytest.raises(ValueError):
            mvfile.unpack(with_u32(off, v))
    with pytest.raises(ValueError):                     # a mode byte more than the header's count
        mvfile.unpack(mvfile.pack(mv, 4, bmv=bmv)[:-4] + struct.pack("<I", 11) + __import__("zlib").compress(b"\0" * 13, 6)[:11])
    for bad in (mv + np.float32(0.125), mv * np.float32(1e6), np.full_like(mv, np.nan)):
        with pytest.raises(ValueError):
            mvfile.pack(bad, 4)
    with pytest.raises(ValueError):
        mvfile.pack(mv, 2)                              # quarter-pel vectors off the half-pel grid
    with pytest.raises(ValueError):
        mvfile.pack(mv, 4, bmv=bmv, modes=modes[:, :2])


# ---- the refinement's properties ----------------------------------------------------------------

def shifted_pair(H, W, dx, dy, seed):
    """(ref, cur) of noise with cur[y, x] = ref[y + dy, x + dx] wherever that lies in the frame."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = max(abs(dx), abs(dy))
    canvas = rng.integers(0, 256, (H + 2 * m, W + 2 * m, 3), dtype=np.uint8)
    return canvas[m:m + H, m:m + W].copy(), canvas[m + dy:m + dy + H, m + dx:m + dx + W].copy()


def restore_case(bs=8, seed=3):
    """The true field of a pair shifted by (3, -2) (zero where that vector is invalid) with scattered
    blocks zeroed -> (ref, cur, field, truth)."""
    H, W = 6 * bs + 3, 7 * bs + 5
    ref, cur = shifted_pair(H, W, 3, -2, seed)
    truth = np.zeros((H // bs, W // bs, 2), np.float32)
    for by in range(H // bs):
        for bx in range(W // bs):
            if R.valid(4 * bx * bs + 12, 4 * by * bs - 8, bs, H, W):
                truth[by, bx] = (3, -2)
    field = truth.copy()
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    field[rng.random(truth.shape[:2]) < 0.3] = 0
    field[2:4, 2:4] = 0            # a hole whose inside has no correct neighbour
    return ref, cur, field, truth


def check_restored(out, field, truth):
    nby, nbx = truth.shape[:2]
    seen = 0
    for by in range(nby):
        for bx in range(nbx):
            t = tuple(truth[by, bx])
            if t == (0, 0):
                continue
            if tuple(field[by, bx]) == t:
                assert tuple(out[by, bx]) == t, (by, bx)             # SAD 0 at index 0
                continue
            near = [(by, bx - 1), (by - 1, bx), (by, bx + 1), (by + 1, bx)]
            if any(0 <= y < nby and 0 <= x < nbx and tuple(field[y, x]) == t for y, x in near):
                assert tuple(out[by, bx]) == t, (by, bx)
                seen += 1
    assert seen >= 5
    assert tuple(out[2, 2]) != tuple(truth[2, 2]) or tuple(field[1, 2]) == (3, -2) or tuple(field[2, 1]) == (3, -2)


def tie_case(bs=8, subpel=4, seed=4):
    """Constant frames and a random field on the 1/subpel grid whose vectors are valid at every block
    (non-negative, inside a margin beyond the full blocks), so that every predictor is valid too."""
    nby, nbx, margin = 5, 6, 4
    H, W = nby * bs + margin, nbx * bs + margin
    frame = np.full((H, W, 3), 77, np.uint8)
    rng = np.random.Generator(np.random.PCG64(seed))
    step = 4 // subpel
    q = rng.integers(0, (4 * (margin - 1)) // step + 1, (nby, nbx, 2)) * step
    q[rng.random((nby, nbx)) < 0.3] = q[0, 0]              # repeated vectors: blocks whose predictor is their own
    return frame, frame.copy(), (q / 4.0).astype(np.float32)


def check_tie_rule(out, field):
    """lambda = 1 on constant frames: J = R(c, p), least (2 bits) at c = p alone; p sits at index 1, so
    a block keeps its own vector only when that is p."""
    F = M.quarter_pels(field)
    moved = 0
    for by in range(F.shape[0]):
        for bx in range(F.shape[1]):
            p = M.predictor(F, by, bx)
            assert tuple(int(v) for v in np.rint(out[by, bx] * 4)) == p, (by, bx)
            moved += p != tuple(F[by, bx])
    assert 5 <= moved < F.shape[0] * F.shape[1]


def test_refinement_restores_zeroed_blocks_at_lambda_0():
    ref, cur, field, truth = restore_case()
    check_restored(M.refine(ref, cur, field, 8, 1, 0, 1), field, truth)


@pytest.mark.parametrize("subpel", [1, 4])
def test_refinement_tie_rule(subpel):
    ref, cur, field = tie_case(subpel=subpel)
    check_tie_rule(M.refine(ref, cur, field, 8, subpel, 1, 1), field)


def test_refinement_restatement_edges():
    rng = np.random.Generator(np.random.PCG64(8))
    ref, cur = (rng.integers(0, 256, (20, 28, 3), dtype=np.uint8) for _ in range(2))
    f = np.array([[[np.nan, 1e30], [-np.inf, 0.25], [100.0, -100.0]]], np.float32)
    assert M.quarter_pels(f).tolist() == [[[-(1 << 28), 1 << 28], [-(1 << 28), 1], [400, -400]]]
    out = M.refine(ref, cur, np.repeat(f, 2, 0), 8, 4, 37, 2)
    assert np.all(np.isfinite(out)) and np.all(np.abs(out) <= 28)          # winners are valid vectors
    assert M.rate((1 << 28, -(1 << 28)), (-(1 << 28), 1 << 28), 1) == 122    # the bound of R
    assert M.refine(ref, cur, np.zeros((0, 3, 2), np.float32), 32, 1, 0, 1).shape == (0, 3, 2)
    assert M.cdiv(-7, 2) == -3 and M.cdiv(7, 2) == 3 and M.cdiv(-8, 4) == -2


# ---- the codec --------------------------------------------------------------------------------

def test_parser_flags():
    from vcf_amd.codec import parser as P
    a = P.parse(P.ipp_parser(), ["encode", "-i", "x", "-O", "y"])
    assert a.mvc is False and a.mv_lambda == 0 and a.mv_iters == 2
    a = P.parse(P.ipp_parser(), ["encode", "-i", "x", "-O", "y", "--mvc", "--mv_lambda", "16", "--mv_iters", "3"])
    assert a.mvc is True and a.mv_lambda == 16 and a.mv_iters == 3
    for bad in (["--mv_iters", "0"], ["--mv_iters", "5"], ["--mv_lambda", "1.5"]):
        with pytest.raises(SystemExit):
            P.parse(P.ipp_parser(), ["encode", "-i", "x", "-O", "y"] + bad)


def test_wrappers_reject_before_any_device_work():
    f = np.zeros((32, 32, 3), np.uint8)
    mv = np.zeros((2, 2, 2), np.float32)
    for kw in (dict(lam=-1), dict(lam=1025), dict(lam=1.5), dict(lam=True), dict(iterations=0), dict(iterations=5),
               dict(subpel=3)):
        with pytest.raises(ValueError):
            K.refine_field(f, f, mv, 16, **kw)
    with pytest.raises(ValueError):
        K.refine_field(f, f, mv[:1], 16)
    with pytest.raises(ValueError):
        K.refine_field(f, f, mv, 65)
    with pytest.raises(ValueError):
        K.refine_field(f, f[:16], mv, 16)
    assert K.refine_field(f[:8], f[:8], np.zeros((0, 2, 2), np.float32), 16).shape == (0, 2, 2)   # an empty field


_A, _M = 0x10000, 0x10001


def test_argument_errors_come_before_any_device_work():
    """Made-up addresses: validation fails first, so nothing is touched and no GPU is needed."""
    lib = L.lib()
    n = ctypes.c_int64()
    assert lib.vcf_ipp_mv_refine_workspace_bytes(37, 50, 8, ctypes.byref(n)) == L.VCF_OK
    assert n.value == 2 * 37 * 50 + 3 + 8 * 4 * 6
    for a in ((0, 50, 8), (37, -1, 8), (37, 50, 0), (37, 50, 65)):
        assert lib.vcf_ipp_mv_refine_workspace_bytes(*a, ctypes.byref(n)) == L.VCF_ERR_INVALID
    assert lib.vcf_ipp_mv_refine_workspace_bytes(37, 50, 8, None) == L.VCF_ERR_INVALID
    good = dict(ref=_A, cur=_A, H=37, W=50, bs=8, subpel=4, lam=8, it=2, mv=_A, ws=_M, nws=n.value)

    def rc(**kw):
        a = {**good, **kw}
        return lib.vcf_ipp_mv_refine(a["ref"], a["cur"], a["H"], a["W"], a["bs"], a["subpel"], a["lam"], a["it"], a["mv"],
                                     a["ws"], a["nws"], None)
    for kw in (dict(ref=None), dict(cur=None), dict(mv=None), dict(ws=None), dict(H=0), dict(W=-3), dict(bs=0), dict(bs=65),
               dict(subpel=0), dict(subpel=3), dict(subpel=8), dict(lam=-1), dict(lam=1025), dict(it=0), dict(it=5),
               dict(nws=n.value - 1), dict(nws=0), dict(H=65536 * 2, W=2, bs=1, nws=1 << 40)):
        assert rc(**kw) == L.VCF_ERR_INVALID, kw
        assert lib.vcf_last_error()
    for off in (1, 2, 3):
        assert rc(mv=_A + off) == L.VCF_ERR_INVALID
        assert b"aligned" in lib.vcf_last_error()


REFINED = []


def _tools():
    t = T._tools()

    def refine_field(ref, cur, mv, bs, subpel=1, lam=0, iterations=2):
        REFINED.append((subpel, lam, iterations))
        return M.refine(ref, cur, mv, bs, subpel, lam, iterations)
    t.refine_field = refine_field
    return t


def _encode(monkeypatch, tmp_path, name, extra):
    import vcf_amd.codec.ipp as C
    from vcf_amd.codec import parser as P
    monkeypatch.setattr(C, "K", _tools())
    src = tmp_path / "frames.npy"
    if not src.exists():
        np.save(src, np.stack(R.subpel_sequence(T.SEQ["H"], T.SEQ["W"], T.SEQ["n"], seed=T.SEQ["seed"])))
    prefix = str(tmp_path / name / "v")
    enc = T._stand_in(C)(P.parse(P.ipp_parser(), ["encode", "-i", str(src), "-O", prefix, "-N", str(T.SEQ["n"]), "-G",
                                                 str(T.SEQ["gop"]), "-S", "2", "-M", "16"] + extra))
    bits = enc.encode()
    return json.load(open(prefix + "_meta.json")), prefix, enc, bits


@pytest.mark.parametrize("extra", [[], ["--subpel", "4"], ["--bframes", "1"], ["-R", "0.5"]],
                         ids=["alone", "subpel4", "bframes1", "R"])
def test_codec_over_numpy_tools(monkeypatch, tmp_path, extra):
    import os
    plain, p0, e0, bits0 = _encode(monkeypatch, tmp_path, "a", extra)
    meta, p1, e1, bits1 = _encode(monkeypatch, tmp_path, "b", extra + ["--mvc"])
    assert "mv_codec" not in plain and plain["mv_file"] == "v_mv.npz"
    assert meta["mv_codec"] == "median-eg0" and meta["mv_file"] == "v_mv.vmv"
    assert set(meta) == set(plain) | {"mv_codec"}
    assert os.path.exists(p1 + "_mv.vmv") and not os.path.exists(p1 + "_mv.npz")
    # the same frames, and the file counted in total_bits exactly as the .npz is
    assert bits1 - 8 * os.path.getsize(p1 + "_mv.vmv") == bits0 - 8 * os.path.getsize(p0 + "_mv.npz")
    assert meta["total_bits"] == bits1
    with np.load(p0 + "_mv.npz", allow_pickle=False) as z:
        f = mvfile.read(p1 + "_mv.vmv")
        assert np.array_equal(f["mv_f32"], z["mv_f32"])
        if "bmv_f32" in z.files:
            assert np.array_equal(f["bmv_f32"], z["bmv_f32"]) and np.array_equal(f["modes"], z["bmodes_u8"])
        elif "modes_u8" in z.files:
            assert np.array_equal(f["modes"], z["modes_u8"])
        else:
            assert f["modes"] is None and f["bmv_f32"] is None
    a, b = T._decode(tmp_path, p0), T._decode(tmp_path, p1)
    assert len(a) == T.SEQ["n"] and all(np.array_equal(x, y) for x, y in zip(a, b))
    # --mv_lambda: every search is followed by the refinement, and the decoder still reproduces the encoder
    del REFINED[:]
    meta2, p2, e2, _ = _encode(monkeypatch, tmp_path, "c", extra + ["--mvc", "--mv_lambda", "64", "--mv_iters", "1"])
    assert set(meta2) == set(meta)
    subpel = 4 if "--subpel" in extra else 1
    assert REFINED == [(subpel, 64, 1)] * (len(meta2["P_info"]) + 2 * len(meta2.get("B_info", [])))
    del REFINED[:]
    got = T._decode(tmp_path, p2)
    kept = [i for i, t in enumerate(meta2.get("frame_types", "IPPIP")) if t != "B"]
    assert len(e2.encoder_recon) == len(kept)
    for k, i in enumerate(kept):
        assert np.array_equal(got[i], e2.encoder_recon[k]), i


def test_decoder_checks_the_motion_file(monkeypatch, tmp_path):
    meta, prefix, _, _ = _encode(monkeypatch, tmp_path, "e", ["--mvc", "--subpel", "2"])
    T._decode(tmp_path, prefix)

    def rewrite(**kw):
        with open(prefix + "_meta.json", "w") as f:
            json.dump({**meta, **kw}, f)
    for kw in (dict(subpel=4), dict(height=meta["height"] + 16), dict(width=meta["width"] - 16),
               dict(P_info=meta["P_info"][:-1])):
        rewrite(**kw)
        with pytest.raises(ValueError, match="header disagrees"):
            T._decode(tmp_path, prefix)
    rewrite(mv_codec="other")
    with pytest.raises(NotImplementedError, match="mv_codec"):
        T._decode(tmp_path, prefix)
    rewrite()
    with open(prefix + "_mv.vmv", "ab") as f:
        f.write(b"\0")
    with pytest.raises(ValueError, match="after the last stream"):
        T._decode(tmp_path, prefix)


def test_refusals(tmp_path):
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec
    for bad in (["--mv_lambda", "1025"], ["--mv_lambda", "-1"]):
        with pytest.raises(ValueError, match="mv_lambda"):
            CoDec(P.parse(P.ipp_parser(), ["encode", "-i", "x", "-O", str(tmp_path / "v")] + bad))

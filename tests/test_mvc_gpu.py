"""The rate-aware refinement of a motion field on the GPU
(vcf_amd/csrc/vcf_ipp_mvrefine.hip) against the numpy restatement of the rule
(tests/mvc_ref.py): the kernel bit for bit, its two properties, pointer
alignment and written extents, a caller's stream, and --mvc / --mv_lambda
through the IPP codec end to end."""
import ctypes
import filecmp
import hashlib
import json
import os

import numpy as np
import pytest
from PIL import Image

import mvc_ref as M
import subpel_ref as R
import test_mvc as T
from abi_buffers import Guarded
from conftest import GOLDEN
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NULL = ctypes.c_void_p(0)
ENTRY = "vcf_ipp_mv_refine"
SHAPES = [(48, 80, 16),
          (21, 43, 4),        # a border outside the blocks, rows that are no multiple of 4 bytes
          (37, 50, 8),
          (64, 128, 64),
          (16, 16, 16),       # one block
          (10, 12, 16)]       # an empty field
# every subpel x every lambda, the iteration counts in turn
SETTINGS = [(subpel, lam, (1, 2, 4)[(a + b) % 3]) for a, subpel in enumerate((1, 2, 4))
            for b, lam in enumerate((0, 1, 37, 1024))]


@pytest.fixture(scope="module")
def K():
    from vcf_amd import ipp
    return ipp


@pytest.fixture(scope="module")
def L():
    from vcf_amd import _lib
    from vcf_amd.device import set_device
    set_device(0)
    return _lib


def _pairs(rng, H, W):
    """Two frame pairs: full-range noise (the SAD decides), and nearly flat frames (SADs of a few
    units per pixel, so that the rate term and the tie rule decide)."""
    return {"noise": tuple(rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2)),
            "flat": tuple(rng.integers(126, 130, (H, W, 3), dtype=np.uint8) for _ in range(2))}


def _fields(rng, shape):
    """As tests/test_obmc_gpu.py: multiples of 1/4 within +-40 pixels (many invalid), within +-2.75
    pixels (most valid), and the latter with NaN, +-inf and 1e30 entries."""
    wide = (rng.integers(-160, 161, shape) / 4.0).astype(np.float32)
    near = (rng.integers(-11, 12, shape) / 4.0).astype(np.float32)
    odd = (rng.integers(-11, 12, shape) / 4.0).astype(np.float32)
    flat = odd.reshape(-1)
    for i, v in enumerate((np.nan, np.inf, -np.inf, 1e30, -1e30, np.nan)):
        if flat.size:
            flat[(5 * i + 1) % flat.size] = v
    return {"wide": wide, "near": near, "non-finite": odd}


@pytest.mark.parametrize("H,W,bs", SHAPES)
def test_kernel_equals_the_rule(K, H, W, bs):
    rng = np.random.Generator(np.random.PCG64(1000 * H + W))
    changed = 0
    for kind, (ref, cur) in _pairs(rng, H, W).items():
        for name, mv in _fields(rng, (H // bs, W // bs, 2)).items():
            for subpel, lam, it in SETTINGS:
                got = K.refine_field(ref, cur, mv, bs, subpel, lam, it)
                want = M.refine(ref, cur, mv, bs, subpel, lam, it)
                assert got.dtype == np.float32 and np.array_equal(got, want), (kind, name, subpel, lam, it)
                changed += int(got.size and not np.array_equal(got, mv))
    assert changed or H // bs == 0


def test_word_and_byte_paths_agree(K):
    """bs % 4 == 0 takes whole words for whole-pel candidates: the same field on a frame cropped so
    that rows start at every byte alignment, against the rule."""
    rng = np.random.Generator(np.random.PCG64(12))
    for W in (64, 65, 66, 67):
        ref, cur = _pairs(rng, 40, W)["flat"]
        mv = rng.integers(-3, 4, (5, 8, 2)).astype(np.float32)
        assert np.array_equal(K.refine_field(ref, cur, mv, 8, 1, 4, 2), M.refine(ref, cur, mv, 8, 1, 4, 2)), W


def test_restores_zeroed_blocks_at_lambda_0(K):
    ref, cur, field, truth = T.restore_case()
    T.check_restored(K.refine_field(ref, cur, field, 8, 1, 0, 1), field, truth)


@pytest.mark.parametrize("subpel", [1, 4])
def test_tie_rule(K, subpel):
    ref, cur, field = T.tie_case(subpel=subpel)
    T.check_tie_rule(K.refine_field(ref, cur, field, 8, subpel, 1, 1), field)


# ---- pointers and extents -----------------------------------------------------------------------

def _ws_bytes(L, H, W, bs):
    n = ctypes.c_int64()
    L.call("vcf_ipp_mv_refine_workspace_bytes", H, W, bs, ctypes.byref(n))
    assert n.value == 2 * H * W + 3 + 8 * (H // bs) * (W // bs)
    return n.value


def _guarded_call(L, ref, cur, mv, H, W, bs, subpel=4, lam=8, it=2, f_off=0, ws_off=0, mv_off=0, nws=None, reject=False,
                  null=None):
    """One call on Guarded buffers at the given byte offsets -> the field; guards and extents checked."""
    from vcf_amd.device import synchronize
    nb = mv.shape[0] * mv.shape[1]
    need = _ws_bytes(L, H, W, bs) if 1 <= bs <= 64 else 2 * H * W + 3 + 8 * nb
    gr, gc = Guarded(ref.nbytes, f_off, ref), Guarded(cur.nbytes, (f_off + 1) % 4, cur)
    gm, gw = Guarded(max(mv.nbytes, 8) + 8, mv_off, mv if nb else None), Guarded(need + 16, ws_off)
    ptr = {"ref": gr.ptr, "cur": gc.ptr, "mv": gm.ptr, "ws": gw.ptr}
    if null:
        ptr[null] = NULL
    what = f"{ENTRY} {H}x{W} bs {bs} subpel {subpel} lam {lam} it {it} f+{f_off} ws+{ws_off} mv+{mv_off} null {null}"
    args = (ptr["ref"], ptr["cur"], H, W, bs, subpel, lam, it, ptr["mv"], ptr["ws"], need if nws is None else nws, NULL)
    if reject:
        with pytest.raises(L.VCFInvalidArgument) as e:
            L.call(ENTRY, *args)
        assert e.value.status == L.VCF_ERR_INVALID, what
        synchronize()
        for g in (gr, gc, gm, gw):
            g.check_untouched(what)
        return None
    L.call(ENTRY, *args)
    synchronize()
    got = gm.download(np.float32, nb * 2).reshape(mv.shape).copy() if nb else mv.copy()
    gm.check_outside([(0, nb * 8)], what)
    gm.check(what)
    # the workspace: the two gray planes, then the second field at the first aligned address
    if nb:
        field_at = (-(gw.ptr.value + 2 * H * W)) % 4 + 2 * H * W
        gw.check_outside([(0, 2 * H * W), (field_at, field_at + nb * 8)], what)
        planes = gw.download()[:2 * H * W]
        assert np.array_equal(planes[:H * W].reshape(H, W), O.ipp_gray(ref)), what
        assert np.array_equal(planes[H * W:].reshape(H, W), O.ipp_gray(cur)), what
    else:
        gw.check_outside((), what)
    gw.check(what)
    gr.check_untouched(what)
    gc.check_untouched(what)
    return got


@pytest.mark.parametrize("H,W,bs", [(48, 80, 16), (21, 43, 4), (37, 50, 8), (10, 12, 16)])
def test_pointers_and_extents(L, H, W, bs):
    rng = np.random.Generator(np.random.PCG64(H))
    ref, cur = _pairs(rng, H, W)["flat"]
    mv = (rng.integers(-11, 12, (H // bs, W // bs, 2)) / 4.0).astype(np.float32)
    for it in (1, 2):           # an odd count starts with the copy into the workspace
        want = M.refine(ref, cur, mv, bs, 4, 8, it)
        for f_off in range(4):
            for ws_off in range(4):
                got = _guarded_call(L, ref, cur, mv, H, W, bs, it=it, f_off=f_off, ws_off=ws_off)
                assert np.array_equal(got, want), (it, f_off, ws_off)
    assert np.array_equal(_guarded_call(L, ref, cur, mv, H, W, bs, mv_off=4), M.refine(ref, cur, mv, bs, 4, 8, 2))
    for off in (1, 2, 3):
        _guarded_call(L, ref, cur, mv, H, W, bs, mv_off=off, reject=True)
    for kw in (dict(bs=0), dict(bs=65), dict(subpel=0), dict(subpel=3), dict(lam=-1), dict(lam=1025), dict(it=0),
               dict(it=5), dict(nws=_ws_bytes(L, H, W, bs) - 1)):
        a = dict(bs=bs)
        a.update(kw)
        _guarded_call(L, ref, cur, mv, H, W, a.pop("bs"), reject=True, **a)
    for null in ("ref", "cur", "mv", "ws"):
        _guarded_call(L, ref, cur, mv, H, W, bs, reject=True, null=null)


def test_two_calls_on_a_caller_stream(L):
    from vcf_amd.device import DeviceBuffer, Stream
    H, W, bs = 48, 80, 16
    rng = np.random.Generator(np.random.PCG64(77))
    ref, cur = _pairs(rng, H, W)["flat"]
    fields = [(rng.integers(-11, 12, (3, 5, 2)) / 4.0).astype(np.float32) for _ in range(2)]
    nws = _ws_bytes(L, H, W, bs)
    dr, dc = DeviceBuffer.from_array(ref), DeviceBuffer.from_array(cur)
    dm = [DeviceBuffer.from_array(m) for m in fields]
    dw = DeviceBuffer(nws)             # one workspace: the calls are ordered by the stream
    s = Stream()
    try:
        for m, it in zip(dm, (3, 2)):
            L.call(ENTRY, dr.ptr, dc.ptr, H, W, bs, 4, 16, it, m.ptr, dw.ptr, nws, s.handle)
        s.synchronize()
        got = [m.download(np.empty((3, 5, 2), np.float32)) for m in dm]
    finally:
        for b in [dr, dc, dw] + dm:
            b.free()
        s.close()
    for g, m, it in zip(got, fields, (3, 2)):
        assert np.array_equal(g, M.refine(ref, cur, m, bs, 4, 16, it))


# ---- the codec --------------------------------------------------------------------------------

N, GOP, BS, Q = 4, 4, 16, 32
CONFIGS = {"alone": [], "subpel4": ["--subpel", "4"], "bframes1": ["--bframes", "1"], "me_levels1": ["--me_levels", "1"],
           "obmc": ["--obmc"], "R": ["-R", "0.5"]}


@pytest.fixture(scope="module")
def seq():
    return R.subpel_sequence(96, 128, N, seed=4)


def _write_seq(d, frames):
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(d, f"in_{i:04d}.png"))
    return os.path.join(d, "in_%04d.png")


def _decoded(prefix):
    return [np.asarray(Image.open(f"{prefix}_{i:04d}.png").convert("RGB")) for i in range(N)]


def _classes():
    from vcf_amd.codec.ipp import CoDec, _IPP

    class Host(CoDec):
        encoder_recon = None

        def encode_decode_proxy(self, img, frame_type, seq_idx):     # an override: the frame-by-frame host loop
            return _IPP.encode_decode_proxy(self, img, frame_type, seq_idx)

        def _gop(self, frames, g0, i_idx, p0):
            r = super()._gop(frames, g0, i_idx, p0)
            self.encoder_recon = (self.encoder_recon or []) + list(r[3])
            return r
    return CoDec, Host


def _encode(cls, pat, out, extra):
    from vcf_amd.codec import parser as P
    os.makedirs(os.path.dirname(out))
    enc = cls(P.parse(P.ipp_parser(), ["encode", "-i", pat, "-O", out, "-N", str(N), "-G", str(GOP), "-M", str(BS), "-q",
                                       str(Q)] + extra))
    enc.encode()
    return enc


def _decode(src, out):
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.ipp import CoDec
    assert CoDec(P.parse(P.ipp_parser(), ["decode", "-i", src, "-O", out, "-M", str(BS), "-q", str(Q)])).decode() == N
    return _decoded(out)


def _same_files(a, b, skip=(), has="v_P_0_enc.tif"):
    names = sorted(n for n in os.listdir(a) if n not in skip)
    assert names == sorted(n for n in os.listdir(b) if n not in skip) and has in names
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)


def test_mvc_alone_codes_the_same_frames(tmp_path, seq):
    CoDec, _ = _classes()
    pat = _write_seq(str(tmp_path), seq)
    _encode(CoDec, pat, str(tmp_path / "a" / "v"), [])
    _encode(CoDec, pat, str(tmp_path / "b" / "v"), ["--mvc"])
    assert os.path.exists(tmp_path / "b" / "v_mv.vmv") and not os.path.exists(tmp_path / "b" / "v_mv.npz")
    _same_files(tmp_path / "a", tmp_path / "b", skip=("v_mv.npz", "v_mv.vmv", "v_meta.json"))
    ma, mb = (json.load(open(tmp_path / d / "v_meta.json")) for d in "ab")
    assert mb["mv_codec"] == "median-eg0" and mb["mv_file"] == "v_mv.vmv" and "mv_codec" not in ma
    size = lambda d, n: os.path.getsize(tmp_path / d / n)
    assert mb["total_bits"] - 8 * size("b", "v_mv.vmv") == ma["total_bits"] - 8 * size("a", "v_mv.npz")
    a, b = _decode(str(tmp_path / "a" / "v"), str(tmp_path / "da" / "v")), _decode(str(tmp_path / "b" / "v"),
                                                                                  str(tmp_path / "db" / "v"))
    for i in range(N):
        assert np.array_equal(a[i], b[i]), i
    _same_files(tmp_path / "da", tmp_path / "db", has="v_0003.png")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_mv_lambda_decodes_to_the_encoders_reconstruction(tmp_path, seq, name):
    CoDec, Host = _classes()
    pat = _write_seq(str(tmp_path), seq)
    extra = ["--mvc", "--mv_lambda", "8"] + CONFIGS[name]
    _encode(CoDec, pat, str(tmp_path / "a" / "v"), extra)
    host = _encode(Host, pat, str(tmp_path / "b" / "v"), extra)
    _same_files(tmp_path / "a", tmp_path / "b")                      # the resident loop's files are the host loop's
    meta = json.load(open(tmp_path / "a" / "v_meta.json"))
    got = _decode(str(tmp_path / "a" / "v"), str(tmp_path / "dec" / "v"))
    # the encoder reconstructs what it predicts from: every frame but the B-frames
    kept = [i for i, t in enumerate(meta.get("frame_types", "IPPP")) if t != "B"]
    assert len(host.encoder_recon) == len(kept) >= 2
    for k, i in enumerate(kept):
        assert np.array_equal(got[i], host.encoder_recon[k]), f"frame {i}"
    # the fields are the refinement's: the first P field follows from the plain search's by the rule
    from vcf_amd import ipp as K
    from vcf_amd.codec import mvfile
    subpel = 4 if name == "subpel4" else 1
    first = K.block_matching(host.encoder_recon[0], seq[kept[1]], BS, 8, False, subpel=subpel,
                             levels=1 if name == "me_levels1" else 0)
    want = M.refine(host.encoder_recon[0], seq[kept[1]], first, BS, subpel, 8, 2)
    assert np.array_equal(mvfile.read(str(tmp_path / "a" / "v_mv.vmv"))["mv_f32"][0], want)


def test_device_ipp_takes_mv_lambda(tmp_path, seq):
    """DeviceIPP(mv_lambda=8): every gathered TIFF equals the file CoDec --mv_lambda 8 writes, and the fields agree."""
    from vcf_amd.codec.ipp_device import DeviceIPP
    from vcf_amd.codec import mvfile
    from vcf_amd.device import DeviceBuffer
    CoDec, _ = _classes()
    pat = _write_seq(str(tmp_path), seq)
    enc = str(tmp_path / "enc" / "v")
    _encode(CoDec, pat, enc, ["--mvc", "--mv_lambda", "8", "--subpel", "4"])
    with pytest.raises(ValueError):
        DeviceIPP(None, 0, 1, N, 96, 128, Q, GOP, BS, 8, False, mv_lambda=1025)
    job = DeviceIPP(None, 0, 1, N, 96, 128, Q, GOP, BS, 8, False, subpel=4, mv_lambda=8)
    sizes, got, mvs = job.run(DeviceBuffer.from_array(np.stack(seq)))
    files = [f"{enc}_I_0_enc.tif"] + [f"{enc}_P_{p}_enc.tif" for p in range(N - 1)]
    for i, path in enumerate(files):
        want = open(path, "rb").read()
        assert bytes(got[i]) == want and sizes[i] == len(want), i
    assert np.array_equal(np.stack(mvs), mvfile.read(enc + "_mv.vmv")["mv_f32"])


def _digest(path):
    """A file's SHA-256; of an .npz, that of its arrays (name, dtype, shape, bytes) and its size: the
    zip members carry the time of writing."""
    h = hashlib.sha256()
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            for k in sorted(n for n in z.files if n != "mv"):            # "mv" is the reference's pickled twin
                a = z[k]
                h.update(f"{k} {a.dtype.str} {a.shape} ".encode() + np.ascontiguousarray(a).tobytes())
        h.update(f"size {os.path.getsize(path)}".encode())
    else:
        h.update(open(path, "rb").read())
    return h.hexdigest()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_without_the_flags_the_encode_is_the_parents(tmp_path, seq, name):
    """tests/golden/mvc_parent_sha256.json: the digests of every file the commit before this feature
    wrote for the same frames and flags."""
    CoDec, _ = _classes()
    want = json.load(open(os.path.join(GOLDEN, "mvc_parent_sha256.json")))[name]
    pat = _write_seq(str(tmp_path), seq)
    _encode(CoDec, pat, str(tmp_path / "e" / "v"), CONFIGS[name])
    got = {n: _digest(str(tmp_path / "e" / n)) for n in sorted(os.listdir(tmp_path / "e"))}
    assert got == want

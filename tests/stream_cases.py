"""The rows of the caller-stream tests (tests/test_stream_cases.py on the host,
tests/test_streams_gpu.py on the GPU).

A row is one entry point at the smallest shape that reaches state the library
shares between calls: the two scratch buffers of vcf_dct_any.hip, the library's
own streams (vcf_pipeline.h, taken by the pipelined 2D-DWT and by the GPU
deflate), or a hipMemsetAsync of the entry's own on the caller's stream.  It
holds a `real` input, a `decoy` of the same shape (real rotated by a third of
its length and bitwise inverted, so the two differ nearly everywhere), the
constant inputs next to them, a function that enqueues the call on a stream,
and the expected output of any input.  Expected outputs come from the oracle
(oracle/oracle.py, oracle/plugins.py), zlib, or the numpy restatements under
tests/, never from the library; the library is only asked for host-side
numbers (layouts, bounds, workspace sizes).

The input of a call is ONE byte blob and so is its output: an entry with
several input or output pointers takes them at fixed offsets of the blob
(`Row.spec` names the output's typed pieces), so the tests move, snapshot and
compare every row the same way.  Inputs and expected outputs are built on first
use and kept.
"""
import ctypes
import functools
import zlib

import numpy as np

def decoy_of(a: np.ndarray) -> np.ndarray:
    """`a` rotated by a third of its elements and bitwise inverted (u8: 255 - v)."""
    return np.ascontiguousarray(~np.roll(a.reshape(-1), a.size // 3)).reshape(a.shape)


def noise(shape, seed, dtype=np.uint8):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, shape, dtype=dtype)


def _p(base: int, off: int = 0) -> ctypes.c_void_p:
    return ctypes.c_void_p(base + off)


def _up(n: int, a: int = 16) -> int:
    return (n + a - 1) // a * a


class Row:
    """name; group ("scratch", "library", "memset"); make() -> (real, extras) built once; want(inp) ->
    the list of typed output arrays for the input array `inp`, laid out at the offsets of spec();
    call(L, din, dout, ws, ex, s) enqueues on stream handle s with integer addresses; ws_bytes() the
    caller workspace (0: none); mask(pieces) -> which output bytes are defined (None: all)."""

    def __init__(self, name, group, make, want, call, ws_bytes=None, mask=None, exact=None, decoy=None, note=""):
        self.name, self.group, self.note = name, group, note
        self._make, self._want, self.call = make, want, call
        self._ws_bytes, self._mask, self._exact, self._decoy = ws_bytes, mask, exact, decoy or decoy_of
        self._cache = {}

    # ---- inputs -------------------------------------------------------------------------------
    def _inputs(self):
        if "in" not in self._cache:
            real, extras = self._make()
            real = np.ascontiguousarray(real)
            self._cache["in"] = (real, np.ascontiguousarray(self._decoy(real)), [np.ascontiguousarray(e) for e in extras])
        return self._cache["in"]

    real = property(lambda self: self._inputs()[0])
    decoy = property(lambda self: self._inputs()[1])
    extras = property(lambda self: self._inputs()[2])

    def preload(self, real, decoy, extras, want_bytes, mask, want_decoy):
        """Inputs and the expected bytes of `real` and of `decoy` as another process computed them."""
        self._cache["in"] = (real, decoy, list(extras))
        self._cache["bytes", "real"] = (want_bytes, mask)
        self._cache["bytes", "decoy"] = (want_decoy, None)

    # ---- outputs ------------------------------------------------------------------------------
    def pieces(self, which="real"):
        """The typed output arrays for the real (or decoy) input."""
        key = ("pieces", which)
        if key not in self._cache:
            self._cache[key] = [np.ascontiguousarray(p) for p in self._want(getattr(self, which))]
        return self._cache[key]

    def spec(self):
        """[(byte offset, dtype, shape)] of the output blob; every piece starts 16-byte aligned."""
        out, off = [], 0
        for p in self.pieces():
            out.append((off, p.dtype, p.shape))
            off = _up(off + p.nbytes)
        return out

    def expected(self, which="real"):
        """(bytes of the output blob, bool mask of the bytes the entry defines or None)."""
        key = ("bytes", which)
        if key not in self._cache:
            pieces = self.pieces(which)
            spec = self.spec()
            n = spec[-1][0] + pieces[-1].nbytes
            blob = np.zeros(n, np.uint8)
            mask = np.zeros(n, bool)
            m = self._mask(pieces) if self._mask else [None] * len(pieces)
            for (off, _, _), p, pm in zip(spec, pieces, m):
                blob[off:off + p.nbytes] = p.view(np.uint8).reshape(-1)
                mask[off:off + p.nbytes] = True if pm is None else pm
            self._cache[key] = (blob, None if mask.all() else mask)
        return self._cache[key]

    @property
    def out_bytes(self) -> int:
        return self.expected()[0].size

    def ws_bytes(self) -> int:
        return int(self._ws_bytes()) if self._ws_bytes else 0

    def exact_margin(self):
        """For a row whose reference is a float64 restatement: the least distance of the real input's
        coefficients from a quantizer threshold (the restatement pins the bytes when it is >= 1e-9)."""
        return None if self._exact is None else float(self._exact(self.real))


# ---- generic-B DCT (vcf_dct_any.hip): the decode scratch (every B != 8) and the run-time scratch
# (lengths without a compiled plan: float on encode, double on decode) ---------------------------------
def _O():
    from oracle import oracle as O
    return O


def _dct_enc(name, H, W, B, Q, flags, seed, n=1, note=""):
    def make():
        return noise((n, H, W, 3), seed), []

    def want(inp):
        return [np.stack([_O().encode_frame_b(f, B, Q, flags) for f in inp])]

    def call(L, din, dout, ws, ex, s):
        L.call("vcf_dct_dz_encode_any", _p(din), n, H, W, B, Q, flags, _p(dout), s)
    return Row(name, "scratch", make, want, call, note=note)


def _dct_dec(name, H, W, B, Q, flags, seed, n=1, k32=False, note=""):
    entry = "vcf_dct_dz_decode_k32" if k32 else "vcf_dct_dz_decode_any"

    def make():
        return np.stack([_O().encode_frame_b(f, B, Q, flags, k32=k32) for f in noise((n, H, W, 3), seed)]), []

    def want(inp):
        return [np.stack([_O().decode_frame_b(k, H, W, B, Q, flags) for k in inp])]

    def call(L, din, dout, ws, ex, s):
        L.call(entry, _p(din), n, H, W, B, Q, flags, _p(dout), s)
    return Row(name, "scratch", make, want, call, note=note)


def _dct_raw_dec(name, H, W, B, flags, seed):
    def make():
        c = _O().dct_raw_encode_b(noise((H, W, 3), seed), B, flags)
        return np.clip(np.trunc(c / 3), -32768, 32767).astype(np.int16)[None], []   # another quantizer's int16

    def want(inp):
        return [_O().dct_raw_decode_b(inp[0], H, W, B, flags)[None]]

    def call(L, din, dout, ws, ex, s):
        L.call("vcf_dct_raw_decode", _p(din), 1, H, W, B, flags, _p(dout), s)
    return Row(name, "scratch", make, want, call, note="-p weights cache, run-time plan 13, both scratch buffers")


# ---- pipelined 2D-DWT (vcf_dwt.hip through run_pipelined): bior4.4, l = 3, Q 32, two frames of 2^20
# pixels, pipeline_default's threshold (vcf_dwt.hip:1730) ---------------------------------------------
DWT = dict(H=1024, W=1024, wavelet="bior4.4", levels=3, Q=32, n=2)


def _dwt_rows(tag, H, W, wavelet, levels, Q, n, seed, enc_sched=None, dec_sched=None):
    import vcf_amd.dwt as DW

    def sub(frames):
        return [_O().dwt_encode_frame(f, wavelet, levels, Q) for f in frames]

    def ws_bytes():
        return n * DW.layout(H, W, levels)[2]

    def run(L, name, sched, *args):
        if sched is None:
            L.call(name, *args)
        else:
            L.call_ab(name + "_sched", ctypes.byref(L.DwtSchedule(**sched)), *args)

    def enc_call(L, din, dout, ws, ex, s):
        run(L, "vcf_dwt_dz_encode", enc_sched, _p(din), n, H, W, DW.wavelet_index(wavelet), levels, Q, _p(dout), _p(ws), s)

    def dec_call(L, din, dout, ws, ex, s):
        run(L, "vcf_dwt_dz_decode", dec_sched, _p(din), n, H, W, DW.wavelet_index(wavelet), levels, Q, _p(dout), _p(ws), s)

    enc = Row(f"dwt_encode_{tag}", "library", lambda: (noise((n, H, W, 3), seed), []),
              lambda inp: [np.stack([DW.pack(x, H, W, levels) for x in sub(inp)])], enc_call, ws_bytes)
    dec = Row(f"dwt_decode_{tag}", "library",
              lambda: (np.stack([DW.pack(x, H, W, levels) for x in sub(noise((n, H, W, 3), seed))]), []),
              lambda inp: [np.stack([_O().dwt_decode_frame(DW.unpack(p, H, W, levels), H, W, wavelet, levels, Q)
                                     for p in inp])], dec_call, ws_bytes)
    return [enc, dec]


def dwt_pipeline_runs(n, H, W, wavelet, levels, **_):
    """The conditions of vcf_dwt.hip:1957 / :2041 for a call with enc_pipe = 1 / dec_pipe = 1, from
    vcf_dwt_plan: a fast filter (no level on the separable kernels) and pipeline_default's batch."""
    import vcf_amd.dwt as DW
    enc, dec = DW.plan(H, W, wavelet, levels, n)
    fast = all(k != "separable" for k, _ in enc) and all(not k.startswith("separable") for k, _ in dec)
    return fast and n >= 2 and H * W >= 1 << 20


# ---- GPU deflate and inflate -----------------------------------------------------------------------
# vcf_zlib_strips takes the AuxStreams of its translation unit (vcf_deflate.hip:1950) in every call
# that has a strip at all: the only return in front of it is n_frames == 0 || frame_bytes == 0 (:1937),
# and the side stream is the library's own, so `ss != ms` (:1976, :2003) always holds.  One strip
# would do.  ZSTRIPS = 4 strips of 4096 bytes, two of each parse kind (deflate_cases.lazy_rule), so
# that both sides of the fork have a strip to code: the lazy parse on the caller's stream, K2a / K2b /
# K3 on the side stream.
ZSTRIPS, ZSTRIP, ZLEVEL = 4, 4096, 6


def _zlib_rows():
    from deflate_cases import small_strip_frame
    from vcf_amd import zlib_gpu as Z

    def frame():
        return np.frombuffer(small_strip_frame(ZSTRIP, 2, 2), np.uint8).copy()

    def strips(a):
        return [a[i * ZSTRIP:(i + 1) * ZSTRIP].tobytes() for i in range(ZSTRIPS)]

    def slot():
        return Z.bound(ZSTRIP)

    def deflate_want(inp):
        out = np.zeros((ZSTRIPS, slot()), np.uint8)
        sizes = np.zeros(ZSTRIPS, np.int32)
        for i, b in enumerate(strips(inp)):
            c = zlib.compress(b, ZLEVEL)
            out[i, :len(c)] = np.frombuffer(c, np.uint8)
            sizes[i] = len(c)
        return [out, sizes]

    def deflate_mask(pieces):
        out, sizes = pieces   # a slot's bytes past its stream are the kernel's to leave as it likes
        return [(np.arange(out.shape[1])[None, :] < sizes[:, None]).reshape(-1), None]

    def deflate_call(L, din, dout, ws, ex, s):
        L.call("vcf_zlib_strips", _p(din), 1, ZSTRIPS * ZSTRIP, ZSTRIP, ZLEVEL, _p(dout), slot(),
               _p(dout, _up(ZSTRIPS * slot())), _p(ws), s)

    deflate = Row("zlib_strips", "library", lambda: (frame(), []), deflate_want, deflate_call,
                  lambda: Z.workspace(ZSTRIPS), deflate_mask)

    # vcf_inflate_strips: the input blob is the streams in slots of `slot` bytes, then comp_len
    # (int32 x ZSTRIPS); the offset and output-length tables do not depend on the content (extras)
    def lens_off():
        return _up(ZSTRIPS * slot())

    def inflate_blob(a):
        blob = np.zeros(lens_off() + 4 * ZSTRIPS, np.uint8)
        lens = np.zeros(ZSTRIPS, np.int32)
        for i, b in enumerate(strips(a)):
            c = zlib.compress(b, ZLEVEL)
            blob[i * slot():i * slot() + len(c)] = np.frombuffer(c, np.uint8)
            lens[i] = len(c)
        blob[lens_off():] = lens.view(np.uint8)
        return blob

    def inflate_make():
        tables = np.concatenate([np.arange(ZSTRIPS, dtype=np.int64) * slot(), np.arange(ZSTRIPS, dtype=np.int64) * ZSTRIP])
        return inflate_blob(frame()), [tables, np.full(ZSTRIPS, ZSTRIP, np.int32)]

    def inflate_want(inp):
        lens = inp[lens_off():].view(np.int32)
        raw = [zlib.decompress(inp[i * slot():i * slot() + int(lens[i])].tobytes()) for i in range(ZSTRIPS)]
        return [np.frombuffer(b"".join(raw), np.uint8).reshape(ZSTRIPS, ZSTRIP), np.zeros(ZSTRIPS, np.int32)]

    def inflate_call(L, din, dout, ws, ex, s):
        L.call("vcf_inflate_strips", _p(din), _p(ex[0]), _p(din, lens_off()), ZSTRIPS, _p(dout), _p(ex[0], 8 * ZSTRIPS),
               _p(ex[1]), _p(dout, _up(ZSTRIPS * ZSTRIP)), s)

    # the decoy of an inflate row must be streams too, not inverted streams: those of the deflate row's decoy
    inflate = Row("inflate_strips", "library", inflate_make, inflate_want, inflate_call,
                  decoy=lambda real: inflate_blob(decoy_of(frame())))
    return [deflate, inflate]


# ---- entries that zero their output with hipMemsetAsync on the caller's stream, at shapes of their
# own tests ----------------------------------------------------------------------------------------
def _index_hist():
    n, H, W, rows, cols = 2, 24, 40, 2, 2

    def want(inp):
        out = np.zeros((n, rows * cols, 3, 256), np.uint32)
        h, w = H // rows, W // cols
        for f in range(n):
            for i in range(rows):
                for j in range(cols):
                    cell = inp[f, i * h:(i + 1) * h, j * w:(j + 1) * w]
                    for c in range(3):
                        out[f, i * cols + j, c] = np.bincount(cell[..., c].ravel(), minlength=256)
        return [out]

    def call(L, din, dout, ws, ex, s):
        L.call("vcf_index_hist_u8", _p(din), n, H, W, rows, cols, _p(dout), n * rows * cols * 768, s)
    return Row("index_hist_u8", "memset", lambda: (noise((n, H, W, 3), 61), []), want, call)


def _ssim():
    n, H, W, C = 2, 24, 40, 3

    def make():
        a = noise((n, H, W, C), 62)
        b = np.clip(a.astype(np.int32) + noise(a.shape, 63).astype(np.int32) // 8 - 16, 0, 255).astype(np.uint8)
        return a, [b]

    def want(inp):
        import ssim_ref as R
        from vcf_amd.distortion import SSIM_RECORD
        sum_k, windows, min_k = R.ssim_ref(inp, ssim.extras[0])
        rec = np.zeros((n, C), SSIM_RECORD)
        rec["sum_k"], rec["windows"], rec["min_k"] = sum_k, windows, min_k
        return [rec.view(np.int64).reshape(n, C, 3)]

    def call(L, din, dout, ws, ex, s):
        L.call("vcf_ssim_u8", _p(din), _p(ex[0]), n, H, W, C, _p(dout), s)
    ssim = Row("ssim_u8", "memset", make, want, call)
    return ssim


def _vq_accumulate():
    H, W, C, BS, K = 10, 14, 3, 2, 5

    def make():
        import vq_restated as R
        img = noise((H, W, C), 64)
        X = R.blocks(img, BS)
        cent = np.ascontiguousarray(X[:K].astype(np.float64) + 0.25)
        return img, [np.ascontiguousarray(R.assign(X, cent)[0], np.uint16)]

    def want(inp):
        import vq_restated as R
        sums, counts = R.accumulate(R.blocks(inp, BS), vq.extras[0], K)
        return [np.ascontiguousarray(sums, np.int64), np.ascontiguousarray(counts, np.int64)]

    def call(L, din, dout, ws, ex, s):
        L.call("vcf_vq_accumulate", _p(din), H, W, C, BS, _p(ex[0]), K, _p(dout), _p(dout, _up(K * BS * BS * C * 8)), s)
    vq = Row("vq_accumulate", "memset", make, want, call)
    return vq


def _lm_histogram():
    H, W = 67, 131

    def want(inp):
        from oracle import plugins as P
        return [np.stack([P.histogram(inp[..., c], 0, 255) for c in range(3)]).astype(np.int64)]

    def call(L, din, dout, ws, ex, s):
        L.call("vcf_lm_histogram", _p(din), L.VCF_DTYPE_U8, H * W, 3, 0, 255, _p(dout), s)
    return Row("lm_histogram", "memset", lambda: (noise((H, W, 3), 65), []), want, call)


def _mdct_encode():
    H, W, B, Q = 20, 26, 6, 32

    def want(inp):
        import mdct_restated as M
        return [M.encode(inp[0], B, Q, 0)["k"][None]]

    def exact(inp):
        import mdct_restated as M
        return M.index_margin(M.encode(inp[0], B, Q, 0)["pre"], Q).min()

    def call(L, din, dout, ws, ex, s):
        L.call("vcf_mdct_dz_encode", _p(din), 1, H, W, B, Q, 0, _p(dout), s)
    return Row("mdct_dz_encode", "memset", lambda: (noise((1, H, W, 3), 66), []), want, call, exact=exact)


def _klt_encode():
    H, W, B, Q = 16, 20, 4, 32

    def make():
        import klt_sweep_cases as S
        return noise((1, H, W, 3), 67), [S.weights(B)]

    def want(inp):
        import klt_restated as K
        return [K.encode(inp[0], klt.extras[0], B, Q, 0)["k"][None]]

    def exact(inp):
        import klt_restated as K
        return K.index_margin(K.encode(inp[0], klt.extras[0], B, Q, 0)["pre"], Q).min()

    def call(L, din, dout, ws, ex, s):
        L.call("vcf_klt_dz_encode", _p(din), 1, H, W, B, Q, 0, _p(ex[0]), _p(dout), s)
    klt = Row("klt_dz_encode", "memset", make, want, call, exact=exact)
    return klt


@functools.lru_cache(maxsize=None)
def _tables():
    rows = [
        _dct_dec("dct16_decode_small", 40, 56, 16, 32, 0, 11, note="compiled length: the two-pass decode scratch"),
        _dct_dec("dct16_decode_large", 200, 300, 16, 32, 0, 12, n=3, note="the same scratch, 28 times the bytes"),
        _dct_enc("dct7_encode", 20, 30, 7, 5, 1, 13, note="run-time path: float run-time scratch"),
        _dct_dec("dct7_decode", 20, 30, 7, 5, 1, 13, note="double run-time scratch and the decode scratch"),
        _dct_dec("dct7_decode_k32", 15, 18, 7, 3, 0, 14, n=2, k32=True, note="int32 indices: 4-byte decode scratch"),
        _dct_raw_dec("dct13_raw_decode_p", 27, 40, 13, 2, 15),
        _dct_enc("dct191_encode", 193, 191, 191, 32, 0, 16, note="Bluestein length: the largest run-time scratch"),
    ]
    # the A/B library's _sched twins are the product code under a forced schedule (include/vcf_amd_ab.h)
    rows += _dwt_rows("pipe", DWT["H"], DWT["W"], DWT["wavelet"], DWT["levels"], DWT["Q"], DWT["n"], 77,
                      enc_sched={"enc_pipe": 1}, dec_sched={"dec_pipe": 1})
    rows += _zlib_rows()
    rows += [_index_hist(), _ssim(), _vq_accumulate(), _lm_histogram(), _mdct_encode(), _klt_encode()]
    # not a row of the ordering table: a small frame through the product entry, the first user of a
    # filter bank in test_first_call_of_a_process_on_a_caller_stream
    extra = [_dwt_rows("small", 24, 32, "bior4.4", 2, 32, 2, 78)[0],
             # a compiled-length ENCODE takes no scratch: the first user of the twiddle tables that cannot
             # block the host in Scratch::acquire
             _dct_enc("dct16_encode_small", 40, 56, 16, 32, 0, 17, note="twiddle tables, no scratch"),
             # a run-time length none of the first-call rows uses, at a size that needs more of both
             # scratch buffers than they do (scratch_bytes): run on the idle stream, it grows them beforehand
             _dct_dec("dct17_decode_warm", 68, 85, 17, 5, 0, 18, note="grows both scratch buffers")]
    return tuple(rows), tuple(extra)


def rows():
    return _tables()[0]


def extra_rows():
    return _tables()[1]


def by_name(name):
    return [r for r in rows() + extra_rows() if r.name == name][0]


NAMES = ("dct16_decode_small", "dct16_decode_large", "dct7_encode", "dct7_decode", "dct7_decode_k32",
         "dct13_raw_decode_p", "dct191_encode", "dwt_encode_pipe", "dwt_decode_pipe", "zlib_strips", "inflate_strips",
         "index_hist_u8", "ssim_u8", "vq_accumulate", "lm_histogram", "mdct_dz_encode", "klt_dz_encode")
EXTRA_NAMES = ("dwt_encode_small", "dct16_encode_small", "dct17_decode_warm")
# the first user, in a fresh process, of: the twiddle tables, a run-time plan, the -p weights, the MDCT
# tables, a DWT filter bank, a LloydMax edge table
FIRST_CALL = ("dct16_encode_small", "dct7_encode", "dct13_raw_decode_p", "mdct_dz_encode", "dwt_encode_small",
              "lm_histogram")
# run once on the idle stream after the first of them, so that no later first call has to grow a scratch buffer
# (a growing scratch waits on the host for its last user: the ordering sequence could not be conclusive)
FIRST_CALL_WARM = "dct17_decode_warm"


def scratch_bytes(H, W, B, n=1, decode=False, esz=2, bluestein=False):
    """(decode scratch, run-time scratch) bytes a generic-B DCT call asks Scratch::acquire for, restated
    from vcf_dct_any.hip: any_decode takes Hp * Wp * 3 * esz per frame (esz 2, or 4 for int32 indices);
    a length without a compiled plan takes min(units, 4096) workgroups x (B^2 + rt_line_reals * 256)
    reals, float on encode and double on decode, rt_line_reals = 2 B, or for a Bluestein length
    4 B + 4 n2 with n2 >= 2 B - 1 (vcf_pocketfft_rt.h): for those a lower bound."""
    Hp, Wp = -(-H // B) * B, -(-W // B) * B
    units = n * (Hp // B) * (Wp // B) * 3
    line = 2 * B + ((2 * B + 4 * (2 * B - 1)) if bluestein else 0)
    compiled = B <= 128 and _five_smooth(B)
    rt = 0 if compiled else min(units, 4096) * (B * B + line * 256) * (8 if decode else 4)
    return (n * Hp * Wp * 3 * esz if decode else 0), rt


def _five_smooth(B):
    for q in (2, 3, 5):
        while B % q == 0:
            B //= q
    return B == 1

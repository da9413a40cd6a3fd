"""The batches both batch-split test files run (tests/test_batch_split.py on the
host, tests/test_batch_split_gpu.py on the GPU), and their references.

Every batched launcher of the library cuts a batch into launches of at most
65535 frames (the limit of a grid's y and z dimension) and shifts its pointers
by the first frame of each launch.  A batch that reaches the second launch has
more than 65535 frames, too many to hand to a host reference one by one, so
every batch here repeats a pool of P = 251 distinct frames: frame f holds pool
entry f % 251, per-frame parameters (weights, means, offset tables) included,
and the expected output of frame f is the reference's output for that entry,
computed once per entry by the references the suite already has.  251 is prime
and 65535 % 251 = 24, so frame f of the second launch holds neither what frame
f - 65535 holds nor what frame f % 65535 holds: a launch that starts at the
wrong frame, or a per-frame table shifted by the wrong stride, shows.
N = 65535 + 24 + 3 frames cross the split and leave a short, odd second launch.

The tiled CBAAC and DWT entries refuse a batch past the grid limit instead of
splitting it; they get the largest batch they take, of the same construction.

any_decode (vcf_dct_any.hip) splits by workspace instead: ANY_B holds the
shapes whose int16 / int32 workspace passes 1 GiB, and chunk_frames() restates
the launcher's rule.
"""
import functools
import zlib

import numpy as np

import klt_restated as K
import lbt_restated as R
import mdct_restated as M
import ssim_ref
from oracle import oracle as O

P = 251
SPLIT = 65535
N = SPLIT + SPLIT % P + 3
PROBES = (0, SPLIT - 1, SPLIT, SPLIT + 1, N - 1)


def entry_of(n=N):
    """The pool entry of every frame of a batch of n."""
    return np.arange(n) % P


def batch(pool, n=N):
    """Frame f = pool[f % P]; the same for an expected pool."""
    pool = np.asarray(pool)
    assert pool.shape[0] == P
    return np.take(pool, entry_of(n), axis=0)


def _ro(a):
    a.setflags(write=False)
    return a


def _frozen(d):
    return {k: _ro(np.ascontiguousarray(v)) for k, v in d.items()}


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def pairwise_distinct(pool):
    """True when no two entries of a pool (first axis) are equal."""
    pool = np.ascontiguousarray(pool)
    return len({pool[i].tobytes() for i in range(pool.shape[0])}) == pool.shape[0]


def _frames(seed, H, W, C=3):
    return _rng(seed).integers(0, 256, (P, H, W, C), dtype=np.uint8)


# ---- 8 x 8 DCT ---------------------------------------------------------------------------
# 8 x 8 is one block, 5 x 7 the PAD instantiations; Q = 32 the packed-fp32 kernels, Q = 7 the scalar ones
DCT = [dict(name=f"{H}x{W}_q{Q}{'_x' if flags else ''}", H=H, W=W, Q=Q, flags=flags)
       for H, W in ((8, 8), (5, 7)) for Q in (32, 7) for flags in (0, O.FLAG_NO_SUBBANDS)]
DCT_IDS = [c["name"] for c in DCT]
DCT_DECODE_VARIANTS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def dct(name):
    """dict(rgb, k, decoded): the pool's frames, the oracle's indices and the oracle's decode of them."""
    c = [c for c in DCT if c["name"] == name][0]
    rgb = _frames(1000 + 8 * c["H"] + c["W"], c["H"], c["W"])
    k = np.stack([O.encode_frame(f, c["Q"], c["flags"]) for f in rgb])
    dec = np.stack([O.decode_frame(x, c["H"], c["W"], c["Q"], c["flags"]) for x in k])
    return _frozen(dict(rgb=rgb, k=k, decoded=dec))


# ---- 2D-MDCT -------------------------------------------------------------------------------
# B = 2 is the smallest block size; a 3 x 5 frame pads to 8 x 10 (one block of context each side)
MDCT = dict(B=2, H=3, W=5, Q=5, flags=0)


@functools.lru_cache(maxsize=None)
def mdct():
    """dict(rgb, k, k_pre, decoded, decoded_pre) of the float64 restatement."""
    c = MDCT
    rgb = _frames(2000, c["H"], c["W"])
    e = [M.encode(f, c["B"], c["Q"], c["flags"]) for f in rgb]
    k = np.stack([x["k"] for x in e])
    d = [M.decode(x, c["H"], c["W"], c["B"], c["Q"], c["flags"]) for x in k]
    return _frozen(dict(rgb=rgb, k=k, k_pre=np.stack([x["pre"] for x in e]), decoded=np.stack([x["rgb"] for x in d]),
                        decoded_pre=np.stack([x["pre"] for x in d])))


# ---- 2D-KLT and 2D-LBT: B = 2 on 3 x 5 frames (padded to 4 x 6: six blocks) -----------------
BLOCK = dict(B=2, H=3, W=5, Q=8)


def _orthonormal(rng, shape):
    return np.linalg.qr(rng.normal(size=shape))[0]


@functools.lru_cache(maxsize=None)
def klt(flags=0):
    """dict(rgb, w64, w32, S1, S2, k, k_margin, decoded, decoded_margin): every pool entry has its own
    orthonormal weights (3, D, D); the moments are klt_restated's exact ones."""
    B, H, W, Q = (BLOCK[x] for x in "BHWQ")
    D = B * B
    rgb = _frames(3000, H, W)
    w64 = _orthonormal(_rng(3001), (P, 3, D, D))
    w32 = w64.astype(np.float32)
    mom = [K.moments(f, B) for f in rgb]
    e = [K.encode(f, w, B, Q, flags) for f, w in zip(rgb, w64)]
    k = np.stack([x["k"] for x in e])
    d = [K.decode(x, H, W, w, B, Q, flags) for x, w in zip(k, w32)]
    return _frozen(dict(rgb=rgb, w64=w64, w32=w32, S1=np.stack([m[0] for m in mom]), S2=np.stack([m[1] for m in mom]),
                        k=k, k_margin=np.stack([K.index_margin(x["pre"], Q) for x in e]),
                        decoded=np.stack([x["rgb"] for x in d]),
                        decoded_margin=np.stack([K.pixel_margin(x["pre"]) for x in d])))


LBT_EPOCHS = 2
LBT_INIT_STD = 0.02     # the product's initial weights are normal with this deviation


@functools.lru_cache(maxsize=None)
def lbt(flags=0):
    """dict of the pool's frames, per-entry orthonormal encoders `we` with decoders `wd` = their
    transposes and the frames' own means; the restatement's indices and decode (k, k_pre, k_mag,
    decoded, decoded_pre, decoded_mag) and the float64 moments S1, S2."""
    B, H, W, Q = (BLOCK[x] for x in "BHWQ")
    D = B * B
    rng = _rng(4000)
    rgb = rng.integers(0, 256, (P, H, W, 3), dtype=np.uint8)
    # the mean of a 3 x 5 frame is a multiple of 1 / 288: redraw the frames whose mean another has
    while True:
        mean = np.array([R.mean_of(f, B) for f in rgb], np.float32)
        again = [i for i in range(P) if mean[i] in mean[:i]]
        if not again:
            break
        rgb[again] = rng.integers(0, 256, (len(again), H, W, 3), dtype=np.uint8)
    we = _orthonormal(_rng(4001), (P, D, D)).astype(np.float32)
    wd = np.ascontiguousarray(we.transpose(0, 2, 1))
    X = [R.blocks(f, B).astype(np.float64) for f in rgb]
    e = [R.encode(f, w, m, B, Q, flags) for f, w, m in zip(rgb, we, mean)]
    k = np.stack([x["k"] for x in e])
    d = [R.decode(x, H, W, w, m, B, Q, flags) for x, w, m in zip(k, wd, mean)]
    return _frozen(dict(rgb=rgb, we=we, wd=wd, mean=mean, S1=np.stack([x.sum(0) for x in X]),
                        S2=np.stack([x.T @ x for x in X]), k=k, k_pre=np.stack([x["pre"] for x in e]),
                        k_mag=np.stack([x["mag"] for x in e]), decoded=np.stack([x["rgb"] for x in d]),
                        decoded_pre=np.stack([x["pre"] for x in d]), decoded_mag=np.stack([x["mag"] for x in d])))


@functools.lru_cache(maxsize=None)
def lbt_training():
    """dict(we0, wd0, we, wd, d_proxy, mean, rows): per pool entry its own initial matrices, the float64
    row-wise restatement's matrices after LBT_EPOCHS epochs, and how far the restatement's float32 run
    ends from them (lbt_sweep_cases.proxy_distance, the stand-in for a fixture's d_ref)."""
    from lbt_sweep_cases import proxy_distance
    B = BLOCK["B"]
    D = B * B
    rgb = lbt()["rgb"]
    rng = _rng(4002)
    we0 = (rng.standard_normal((P, D, D)) * LBT_INIT_STD).astype(np.float32)
    wd0 = (rng.standard_normal((P, D, D)) * LBT_INIT_STD).astype(np.float32)
    mean = lbt()["mean"]
    we, wd, dp = [], [], []
    for i in range(P):
        Xc = R.centred(rgb[i], B, mean[i]).astype(np.float64)
        (a, b), d = proxy_distance(Xc, we0[i], wd0[i], LBT_EPOCHS)
        we.append(a)
        wd.append(b)
        dp.append(d)
    out = _frozen(dict(we0=we0, wd0=wd0, we=np.stack(we), wd=np.stack(wd), d_proxy=np.array(dp), mean=mean))
    Hp, Wp = R.padded_shape(BLOCK["H"], BLOCK["W"], B)[:2]
    out["rows"] = 3 * (Hp // B) * (Wp // B)
    return out


# ---- distortion and SSIM -------------------------------------------------------------------
DIST_SHAPE = (3, 5, 3)      # 45 bytes a frame: the frames of a batch start at every alignment
SSIM_SHAPE = (11, 11, 1)    # one window, 121 bytes


def _pair(seed, shape):
    """Two pools of frames: random content and the same with noise of a few levels."""
    rng = _rng(seed)
    a = rng.integers(0, 256, (P,) + shape, dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
    return a, b


@functools.lru_cache(maxsize=None)
def distortion():
    """dict(a, b, sse, sad, max_abs): numpy int64 sums per frame and channel."""
    a, b = _pair(5000, DIST_SHAPE)
    d = a.astype(np.int64) - b.astype(np.int64)
    return _frozen(dict(a=a, b=b, sse=(d * d).sum(axis=(1, 2)), sad=np.abs(d).sum(axis=(1, 2)),
                        max_abs=np.abs(d).max(axis=(1, 2))))


@functools.lru_cache(maxsize=None)
def ssim():
    """dict(a, b, sum_k, min_k, windows) of tests/ssim_ref.py."""
    a, b = _pair(6000, SSIM_SHAPE)
    res = [ssim_ref.ssim_ref(x, y) for x, y in zip(a, b)]
    assert {r[1] for r in res} == {1}
    return dict(windows=1, **_frozen(dict(a=a, b=b, sum_k=np.concatenate([r[0] for r in res]),
                                          min_k=np.concatenate([r[2] for r in res]))))


# ---- inflate -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inflate():
    """dict(raw, streams): 251 payloads of 1 to 40 bytes and their zlib streams, so the five offset and
    length tables of a batch differ from strip to strip."""
    rng = _rng(7000)
    raw = [rng.integers(0, 256, 1 + i % 40, dtype=np.uint8).tobytes() for i in range(P)]
    return dict(raw=raw, streams=[zlib.compress(b, 6) for b in raw])


def inflate_batch(n=N):
    """(comp, comp_off, comp_len, out_off, out_len, expected bytes) of n strips, strip s = pool[s % P]."""
    z = inflate()
    e = entry_of(n)
    clen = np.array([len(s) for s in z["streams"]], np.int64)[e]
    olen = np.array([len(b) for b in z["raw"]], np.int64)[e]
    coff = np.concatenate([[0], np.cumsum(clen)[:-1]])
    ooff = np.concatenate([[0], np.cumsum(olen)[:-1]])
    reps = -(-n // P)
    comp = np.frombuffer((b"".join(z["streams"]) * reps)[:int(clen.sum())], np.uint8)
    want = np.frombuffer((b"".join(z["raw"]) * reps)[:int(olen.sum())], np.uint8)
    return comp, coff, clen, ooff, olen, want


# ---- 2D-DWT: the largest batch the entries take --------------------------------------------------
# the DWT kernels put plane = 3 * frame + channel on blockIdx.z and take no more than 65535 planes:
# 21845 frames put the last plane at 65534.  3 x 5 is odd both ways (the level pads to 4 x 6), one
# level is the fewest; haar has 2 taps, db2 4.
DWT_N = SPLIT // 3
DWT = dict(H=3, W=5, L=1, Q=8)
DWT_WAVELETS = ("haar", "db2")


def dwt_pack(subbands, levels):
    """A frame's packed bytes as vcf_dwt_dz_encode writes them: LL (uint16), then LH, HL, HH per level."""
    parts = [np.ascontiguousarray(subbands[f"LL_{levels}"], np.uint16).view(np.uint8).ravel()]
    parts += [np.ascontiguousarray(subbands[f"{s}_{r}"], np.uint8).ravel()
              for r in range(levels, 0, -1) for s in ("LH", "HL", "HH")]
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def dwt(wavelet):
    """dict(rgb, packed, decoded): the oracle's subbands of the pool, packed, and its decode of them."""
    H, W, L, Q = (DWT[x] for x in "HWLQ")
    rgb = _frames(9000, H, W)
    sb = [O.dwt_encode_frame(f, wavelet, L, Q) for f in rgb]
    return _frozen(dict(rgb=rgb, packed=np.stack([dwt_pack(s, L) for s in sb]),
                        decoded=np.stack([O.dwt_decode_frame(s, H, W, wavelet, L, Q) for s in sb])))


# ---- tiled CBAAC: the largest batch the entries take ---------------------------------------------
# the *_frames and *_classes entries put the frame on blockIdx.y and take no more than 65535 frames;
# 65535 % 251 = 24, so the last frame, 65534, holds pool entry 23 and its neighbours in the pool differ.
CBAAC_N = SPLIT
CBAAC_PROBES = (0, 16383, 32768, 49151, SPLIT - 1)      # the frames coded on the host one by one
# 256 symbols is the shortest segment; 261 make two, the second cut short.  Two classes give each
# segment of a frame its own prior row.
CBAAC = dict(n=261, seg_len=256, nclass=2)
# 5 x 9 x 2 in tiles of 4 x 8: four tiles a plane, cropped both ways down to one symbol.  One class:
# a frame's 16 prior rows are 8 KiB, 512 MiB for the batch.
CBAAC2D = dict(shape=(5, 9, 2), tile=(4, 8), nclass=1)
CBAAC_KINDS = ("frames", "classes", "tiled2d")


def _index_like(seed, shape):
    """Symbols as a codec's indices are: around 128, Laplacian, every entry at a width of its own."""
    rng = _rng(seed)
    scale = (1.0 + 4.0 * rng.random(P)).reshape((P,) + (1,) * len(shape))
    return np.clip(np.rint(128 + rng.laplace(0, 1, (P,) + shape) * scale), 0, 255).astype(np.uint8)


def _packed(parts, cap):
    """Per pool entry a list of byte strings -> (sizes (P, parts) int64, the strings back to back in
    rows of cap bytes, zeros behind them)."""
    sizes = np.array([[len(p) for p in e] for e in parts], np.int64)
    payload = np.zeros((P, cap), np.uint8)
    for i, e in enumerate(parts):
        b = np.frombuffer(b"".join(e), np.uint8)
        payload[i, :b.size] = b
    return sizes, payload


@functools.lru_cache(maxsize=None)
def cbaac(kind):
    """dict(sym, prior, sizes, payload) of the host serial coder: the pool's frames, each one's prior
    rows, its segments' (tiles') byte counts and their bytes in a row of the entry's capacity."""
    from vcf_amd import _lib as L
    from vcf_amd import tcbaac as T
    if kind == "tiled2d":
        shape, (th, tw), K = (CBAAC2D[x] for x in ("shape", "tile", "nclass"))
        sym = _index_like(9500, shape)
        prior = [T.prior2d_of(f, th, tw, K) for f in sym]
        parts = [T.host_tiles2d(f, p, th, tw, K) for f, p in zip(sym, prior)]
        cap = int(L.lib().vcf_cbaac_tiled2d_bound(*shape, th, tw))
    else:
        n, seg = CBAAC["n"], CBAAC["seg_len"]
        K = CBAAC["nclass"] if kind == "classes" else 1
        sym = _index_like(9600, (n,))
        prior = [T.prior_of(f, K, seg) for f in sym]
        parts = [T.host_segments_prior(f, p, seg, 0) for f, p in zip(sym, prior)]
        cap = int(L.lib().vcf_cbaac_tiled_bound(n, seg))
    sizes, payload = _packed(parts, cap)
    return _frozen(dict(sym=sym, prior=np.stack(prior), sizes=sizes, payload=payload))


def cbaac_probe(kind, f):
    """Frame f of the batch coded on the host by itself -> its segments' (tiles') bytes."""
    from vcf_amd import tcbaac as T
    frame = cbaac(kind)["sym"][f % P]
    if kind == "tiled2d":
        (th, tw), K = CBAAC2D["tile"], CBAAC2D["nclass"]
        return T.host_tiles2d(frame, T.prior2d_of(frame, th, tw, K), th, tw, K)
    seg = CBAAC["seg_len"]
    K = CBAAC["nclass"] if kind == "classes" else 1
    return T.host_segments_prior(frame, T.prior_of(frame, K, seg), seg, 0)


def cbaac_streams(kind, n):
    """What the batched decoders read for n frames: (every frame's bytes back to back, the offsets of
    its segments in them (n, parts + 1))."""
    ref = cbaac(kind)
    e = entry_of(n)
    sizes = ref["sizes"][e]
    total = sizes.sum(axis=1)
    flat = batch(ref["payload"], n)[np.arange(ref["payload"].shape[1]) < total[:, None]]
    offs = np.zeros((n, sizes.shape[1] + 1), np.int64)
    np.cumsum(sizes, axis=1, out=offs[:, 1:])
    offs += np.concatenate([[0], np.cumsum(total)[:-1]])[:, None]
    return flat, offs


# ---- any-B decode: the workspace chunks ----------------------------------------------------------
ANY_B = 16
ANY_TILE = 32       # the index tile every frame repeats: 2 x 2 blocks
ANY_Q = 32
WS_LIMIT = 1 << 30
# (name, frames, H, W, mode); H and W are multiples of ANY_TILE, so Hp = H and Wp = W
ANY = [
    dict(name="u8_two_frames_of_one_chunk_each", n=2, H=9472, W=9472, mode="u8", chunk=1),
    dict(name="u8_five_frames_in_chunks_of_two", n=5, H=7712, W=7744, mode="u8", chunk=2),
    dict(name="k32_two_frames_of_one_chunk_each", n=2, H=6688, W=6720, mode="k32", chunk=1),
]
ANY_IDS = [c["name"] for c in ANY]


def chunk_frames(n, H, W, B, mode):
    """The frames any_decode (vcf_dct_any.hip) takes per pass: its workspace holds Hp x Wp x 3 elements
    a frame, int16 (int32 in the k32 mode), and stays within 1 GiB."""
    Hp, Wp = O.padded_shape(H, W, B)
    frame_ws = Hp * Wp * 3 * (4 if mode == "k32" else 2)
    return max(1, min(n, WS_LIMIT // frame_ws))


@functools.lru_cache(maxsize=None)
def any_tiles(name):
    """(index tiles, decoded tiles), one pair per frame: with -x the blocks of a frame are independent,
    so a frame that repeats an index tile of whole blocks decodes to the repeated decode of the tile."""
    c = [c for c in ANY if c["name"] == name][0]
    rng = _rng(8000 + ANY_IDS.index(name))
    shape = (c["n"], ANY_TILE, ANY_TILE, 3)
    # about 13 nonzero steps of up to 6 per block and channel: dense indices would clip most pixels
    step = np.where(rng.random(shape) < 0.05, rng.integers(-6, 7, shape), 0)
    if c["mode"] == "k32":
        # the -L synthesis adds no 128: a luma DC of 64 steps (x Q / B = 2 levels) centres the pixels
        step[:, ::ANY_B, ::ANY_B, 0] += 64
    k = step.astype(np.int32) if c["mode"] == "k32" else (128 + step).astype(np.uint8)
    dec = np.stack([O.decode_frame_b(x, ANY_TILE, ANY_TILE, ANY_B, ANY_Q, O.FLAG_NO_SUBBANDS) for x in k])
    return _ro(k), _ro(dec)


def any_frames(name):
    """(index frames, expected pixels) of a case, built by np.tile."""
    c = [c for c in ANY if c["name"] == name][0]
    k, dec = any_tiles(name)
    reps = (1, c["H"] // ANY_TILE, c["W"] // ANY_TILE, 1)
    return np.tile(k, reps), np.tile(dec, reps)

"""The RDOQ rule of include/vcf_amd.h (vcf_dct_dz_encode_rdoq) restated in numpy.

The float32 coefficients are the oracle's own: oracle.ref_numpy's _pad, _from_rgb and _get_subbands
and the two scipy.fft.dct calls of its encode_frame, imported and not copied.  The rule then runs in
float64 on whole arrays: J(k) = d * d + lambda * bits, d = c - Q k, one rounded operation each."""
import numpy as np

from oracle import ref_numpy as RN

B = RN.B


def coefficients(rgb: np.ndarray) -> np.ndarray:
    """Hp x Wp x 3 float32, block layout (coefficient (i, j) of block (y, x) at [8 y + i, 8 x + j])."""
    import scipy.fft as sf
    img = RN._pad(rgb.astype(np.float32))
    img -= RN.OFFSET
    ct = RN._from_rgb(img)
    H, W = ct.shape[:2]
    v = ct.reshape(H // B, B, W // B, B, 3)
    v = sf.dct(v, axis=1, norm="ortho")
    v = sf.dct(v, axis=3, norm="ortho")
    return np.ascontiguousarray(v.reshape(H, W, 3))


def _regions(Hp: int, Wp: int) -> np.ndarray:
    """Region 8 i + j of every position of a block-layout frame."""
    return (np.arange(Hp)[:, None] % B) * B + (np.arange(Wp)[None, :] % B)


def _bits_of(bits: np.ndarray, k: np.ndarray) -> np.ndarray:
    """bits[region][channel][(k + 128) & 255] for a block-layout int32 index frame k."""
    Hp, Wp, _ = k.shape
    r = _regions(Hp, Wp)[:, :, None]
    ch = np.arange(3)[None, None, :]
    return bits[r, ch, (k + 128) & 255]


def cost(c: np.ndarray, k: np.ndarray, Q: int, lam: float, bits: np.ndarray) -> np.ndarray:
    """J per coefficient (float64) of the block-layout indices k."""
    d = c.astype(np.float64) - (np.int32(Q) * k.astype(np.int32)).astype(np.float64)
    return d * d + np.float64(lam) * _bits_of(bits, k)


def decide(c: np.ndarray, Q: int, lam: float, bits: np.ndarray) -> np.ndarray:
    """The rule on block-layout float32 coefficients -> int32 indices before the byte wrap.
    bits: float64 64 x 3 x 256."""
    bits = np.asarray(bits, np.float64).reshape(64, 3, 256)
    k0 = (c / Q).astype(np.int32)                     # ref_numpy._tail: float32 quotient, truncated
    s = np.sign(k0)
    cand = (k0 != 0) & (k0 >= -128) & (k0 <= 127)
    best = k0.copy()
    jb = cost(c, np.where(cand, k0, 0), Q, lam, bits)
    k1 = np.where(cand, k0 - s, 0)
    j1 = cost(c, k1, Q, lam, bits)
    take = cand & (j1 <= jb)
    best = np.where(take, k1, best)
    jb = np.where(take, j1, jb)
    jz = cost(c, np.zeros_like(k0), Q, lam, bits)
    take = cand & (k1 != 0) & (jz <= jb)
    return np.where(take, 0, best).astype(np.int32)


def _layout(a: np.ndarray, subbands: bool) -> np.ndarray:
    return RN._get_subbands(a) if subbands else a


def encode_frame(rgb: np.ndarray, Q: int, lam: float, bits: np.ndarray, subbands: bool = True) -> np.ndarray:
    """One frame through the rule: Hp x Wp x 3 uint8 (k + 128, wrapped), in the layout asked for."""
    k = decide(coefficients(rgb), Q, lam, bits)
    return _layout(k + RN.OFFSET, subbands).astype(np.uint8)


def plain_frame(rgb: np.ndarray, Q: int, subbands: bool = True) -> np.ndarray:
    return RN.encode_frame(rgb, Q, subbands)


def _unlayout(idx: np.ndarray, subbands: bool) -> np.ndarray:
    if not subbands:
        return idx
    Hp, Wp = idx.shape[:2]
    sy, sx = Hp // B, Wp // B
    out = np.empty_like(idx)
    for i in range(B):
        for j in range(B):
            out[i::B, j::B] = idx[i * sy:(i + 1) * sy, j * sx:(j + 1) * sx]
    return out


def total_cost(rgb: np.ndarray, idx: np.ndarray, Q: int, lam: float, bits: np.ndarray, subbands: bool = True) -> float:
    """The modelled sum of J of a uint8 index frame (read as k = byte - 128) under a table."""
    bits = np.asarray(bits, np.float64).reshape(64, 3, 256)
    k = _unlayout(np.asarray(idx), subbands).astype(np.int32) - RN.OFFSET
    return float(cost(coefficients(rgb), k, Q, lam, bits).sum())


def counts_of(idx: np.ndarray) -> np.ndarray:
    """rate.histogram(idx, regions=(8, 8)) of one subband-layout uint8 frame on the host: 64 x 3 x 256 uint32."""
    Hp, Wp = idx.shape[:2]
    sy, sx = Hp // B, Wp // B
    out = np.zeros((64, 3, 256), np.uint32)
    for i in range(B):
        for j in range(B):
            for ch in range(3):
                out[i * B + j, ch] = np.bincount(idx[i * sy:(i + 1) * sy, j * sx:(j + 1) * sx, ch].ravel(), minlength=256)
    return out

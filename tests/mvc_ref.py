"""The coded motion field of include/vcf_amd.h ("Coded motion fields") in plain
Python and numpy: the reference for vcf_mv_encode / vcf_mv_decode (median
prediction, signed exp-Golomb codes) and for vcf_ipp_mv_refine (the rate-aware
re-decision of every block's vector).  Integers throughout; the luma is the
oracle's (oracle.ipp_gray) and the SAD is subpel_ref.block_sad's."""
import numpy as np

import subpel_ref as S
from oracle import oracle as O

MAX_Q = 1 << 15        # |q| of a coded vector
MAX_PREFIX = 17        # zeros in front of a code
CLAMP = 1 << 28        # |q| of a float entry


def check_step(step):
    if step not in (1, 2, 4):
        raise ValueError("step must be 1, 2 or 4")


def median3(a, b, c):
    return sorted((a, b, c))[1]


def predictor(F, by, bx):
    """p(by, bx) of the integer field F (nby, nbx, 2) -> (px, py)."""
    nbx = len(F[0])
    zero = (0, 0)
    A = tuple(int(v) for v in F[by][bx - 1]) if bx > 0 else zero
    if by == 0:
        return A
    B = tuple(int(v) for v in F[by - 1][bx])
    if bx + 1 < nbx:
        C = tuple(int(v) for v in F[by - 1][bx + 1])
    elif bx > 0:
        C = tuple(int(v) for v in F[by - 1][bx - 1])
    else:
        C = zero
    return median3(A[0], B[0], C[0]), median3(A[1], B[1], C[1])


def index(d):
    return 2 * d - 1 if d > 0 else -2 * d


def length(d):
    """len(d) = 2 floor(log2(k + 1)) + 1."""
    return 2 * ((index(d) + 1).bit_length() - 1) + 1


def cdiv(a, b):
    """C's division: truncating toward zero (b > 0)."""
    return a // b if a >= 0 else -((-a) // b)


def rate(q, p, step):
    return length(cdiv(q[0] - p[0], step)) + length(cdiv(q[1] - p[1], step))


def code_bits(d):
    """The code of d as a string of '0' / '1': floor(log2(k + 1)) zeros, then k + 1 in binary."""
    v = index(d) + 1
    return "0" * (v.bit_length() - 1) + format(v, "b")


def encode(q, step):
    """(nby, nbx, 2) integers on the step grid -> the stream's bytes."""
    check_step(step)
    q = np.asarray(q)
    nby, nbx = q.shape[:2]
    bits = []
    for by in range(nby):
        for bx in range(nbx):
            p = predictor(q, by, bx)
            for c in range(2):
                v = int(q[by, bx, c])
                if abs(v) > MAX_Q or v % step:
                    raise ValueError(f"vector component {v}")
                bits.append(code_bits(cdiv(v - p[c], step)))
    s = "".join(bits)
    s += "0" * (-len(s) % 8)
    return bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8))


def decode(data, nby, nbx, step):
    """The inverse; ValueError for every stream the encoder does not write."""
    check_step(step)
    s = "".join(format(b, "08b") for b in data)
    pos = 0
    q = [[[0, 0] for _ in range(nbx)] for _ in range(nby)]
    for by in range(nby):
        for bx in range(nbx):
            p = predictor(q, by, bx)
            for c in range(2):
                z = 0
                while pos < len(s) and s[pos] == "0":
                    z, pos = z + 1, pos + 1
                    if z > MAX_PREFIX:
                        raise ValueError("a prefix of more than 17 zeros")
                if pos + z + 1 > len(s):
                    raise ValueError("the stream ends inside a code")
                k = int(s[pos:pos + z + 1], 2) - 1
                pos += z + 1
                d = (k + 1) // 2 if k & 1 else -(k // 2)
                q[by][bx][c] = p[c] + d * step
            if max(abs(v) for v in q[by][bx]) > MAX_Q:
                raise ValueError("a vector beyond +-2^15")
    if (pos + 7) // 8 != len(data):
        raise ValueError("bytes after the last code")
    if "1" in s[pos:]:
        raise ValueError("padding bits set")
    return np.array(q, np.int32).reshape(nby, nbx, 2)


def quarter_pels(mv):
    """A float32 field -> quarter pels: rint(4 m) (half to even), clamped to +-2^28, a NaN -> -2^28."""
    m = np.asarray(mv, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.float32(4) * m).astype(np.float64)
    r = np.where(np.isnan(r), -float(CLAMP), np.clip(r, -CLAMP, CLAMP))
    return r.astype(np.int64)


def refine_once(rg, cg, F, bs, step, lam):
    """One pass on luma planes rg, cg: the integer field F (nby, nbx, 2) -> the winners."""
    H, W = rg.shape
    nby, nbx = F.shape[:2]
    out = np.zeros_like(F)
    for by in range(nby):
        for bx in range(nbx):
            i, j = by * bs, bx * bs
            p = predictor(F, by, bx)
            at = lambda y, x: (int(F[y, x, 0]), int(F[y, x, 1]))
            cands = [at(by, bx), p,
                     at(by, bx - 1) if bx > 0 else None,
                     at(by - 1, bx) if by > 0 else None,
                     at(by, bx + 1) if bx + 1 < nbx else None,
                     at(by + 1, bx) if by + 1 < nby else None,
                     (0, 0)]
            best = None
            for c in cands:
                if c is None or not S.valid(4 * j + c[0], 4 * i + c[1], bs, H, W):
                    continue
                J = S.block_sad(rg, cg, i, j, 4 * j + c[0], 4 * i + c[1], bs) + lam * rate(c, p, step)
                if best is None or J < best:          # the first strict minimum: argmin of (J, index)
                    best, out[by, bx] = J, c
    return out


def refine(ref, cur, mv, bs, subpel=1, lam=0, iterations=2):
    """vcf_ipp_mv_refine: (H//bs, W//bs, 2) float32 in -> float32 out."""
    if subpel not in (1, 2, 4) or not 0 <= lam <= 1024 or not 1 <= iterations <= 4:
        raise ValueError("bad arguments")
    mv = np.asarray(mv, np.float32)
    if mv.size == 0:
        return mv.copy()
    rg, cg = O.ipp_gray(ref), O.ipp_gray(cur)
    F = quarter_pels(mv)
    for _ in range(iterations):
        F = refine_once(rg, cg, F, bs, 4 // subpel, lam)
    return (F / 4.0).astype(np.float32)

"""The vector quantizer restated in numpy and Python integers, from the text of
include/vcf_amd.h (vcf_vq_*): block extraction, assign, accumulate, the
k-means++ init, the Lloyd fit, VQ.py's energy reorder and the decode.  It is
what the GPU tests compare the library with, and what the golden maker checks
against sklearn.  Nothing here imports the package under test."""
import math

import numpy as np

MASK = (1 << 64) - 1
STRICT, TOL, MAX_ITER = "strict", "tol", "max_iter"


def blocks(img, BS):
    """(N, D) int64: block (by, bx) in raster order, img[y:y+BS, x:x+BS, :] flattened (VQ.py:70-74)."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    H, W, C = img.shape
    assert H % BS == 0 and W % BS == 0
    x = img.reshape(H // BS, BS, W // BS, BS, C).transpose(0, 2, 1, 3, 4)
    return np.ascontiguousarray(x).reshape(-1, BS * BS * C).astype(np.int64)


def gamma(D):
    """The dot-product rounding bound of a D-term squared distance of u8 data: 4 * D * 2^-52 * (255^2 * D)."""
    return 4.0 * D * 2.0 ** -52 * (255.0 ** 2 * D)


def distances(X, cent):
    """(N, K) float64: acc = acc + (x_d - c_jd) * (x_d - c_jd), d ascending, each operation rounded."""
    X = np.asarray(X, np.float64)
    cent = np.asarray(cent, np.float64)
    acc = np.zeros((X.shape[0], cent.shape[0]), np.float64)
    for d in range(X.shape[1]):
        t = X[:, d, None] - cent[None, :, d]
        acc = acc + t * t
    return acc


def assign(X, cent):
    """(labels uint16, least distance, gap to the second-best distance [inf when K = 1])."""
    dist = distances(X, cent)
    labels = np.argmin(dist, axis=1)          # the first minimum: the lowest j on a tie
    best = dist[np.arange(dist.shape[0]), labels]
    if dist.shape[1] > 1:
        gap = np.partition(dist, 1, axis=1)[:, 1] - best
    else:
        gap = np.full(dist.shape[0], np.inf)
    return labels.astype(np.uint16), best, gap


def accumulate(X, labels, K):
    sums = np.zeros((K, X.shape[1]), np.int64)
    counts = np.zeros(K, np.int64)
    ok = np.asarray(labels) < K
    np.add.at(sums, np.asarray(labels)[ok], X[ok])
    np.add.at(counts, np.asarray(labels)[ok], 1)
    return sums, counts


def draw(seed, step, trial):
    """splitmix64's output function of seed + golden * (16 * step + trial + 1)."""
    z = (seed + 0x9E3779B97F4A7C15 * (16 * step + trial + 1)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def mulhi64(a, b):
    return (a * b) >> 64


def _sqdist(X, i):
    t = X - X[i]
    return np.sum(t * t, axis=1)      # int64, exact


def init_pp(X, K, seed):
    """Greedy k-means++ in integers: (centroids (K, D) float64, the chosen indices)."""
    N = X.shape[0]
    T = 2 + int(math.log(K))
    ids = [mulhi64(draw(seed, 0, 0), N)]
    closest = _sqdist(X, ids[0])
    for c in range(1, K):
        pot = int(closest.sum())
        run = np.cumsum(closest)
        best = None
        for t in range(T):
            if pot > 0:
                r = mulhi64(draw(seed, c, t), pot)
                cand = int(np.searchsorted(run, r, side="right"))    # the first index whose running sum exceeds r
            else:
                cand = 0
            m = np.minimum(closest, _sqdist(X, cand))
            p = int(m.sum())
            if best is None or p < best[0]:
                best = (p, cand, m)
        ids.append(best[1])
        closest = best[2]
    ids = np.array(ids, np.int64)
    return X[ids].astype(np.float64), ids


def tol_abs(X, tol):
    N, D = X.shape
    total = 0.0
    for d in range(D):
        col = [int(v) for v in X[:, d]]
        s1, s2 = sum(col), sum(v * v for v in col)
        total = total + float(N * s2 - s1 * s1) / float(N * N)
    return tol * (total / D)


def fit(X, K, seed=0, max_iter=300, tol=1e-4, init=None, gaps=None):
    """sklearn's _kmeans_single_lloyd as vcf_vq_fit runs it: (centroids, labels uint16, report dict).
    `gaps`, a list, receives the least best-to-second-best gap of every assign."""
    N, D = X.shape
    cent = np.array(init, np.float64).reshape(K, D) if init is not None else init_pp(X, K, seed)[0]
    ta = tol_abs(X, tol)
    old = None
    reason, n_iter, relocations = MAX_ITER, 0, 0
    for it in range(max_iter):
        labels, best, gap = assign(X, cent)
        if gaps is not None:
            gaps.append(float(gap.min()))
        sums, counts = accumulate(X, labels, K)
        empty = np.flatnonzero(counts == 0)
        if empty.size:
            order = sorted(range(N), key=lambda n: (-best[n], n))
            for i, to in enumerate(empty[:N]):
                far = order[i]
                if not best[far] > 0.0:
                    break
                frm = int(labels[far])
                sums[frm] -= X[far]
                sums[to] = X[far]
                counts[to] = 1
                counts[frm] -= 1
                relocations += 1
        fresh = cent.copy()
        live = counts > 0
        fresh[live] = sums[live].astype(np.float64) / counts[live].astype(np.float64)[:, None]
        shift = 0.0
        for v in ((fresh - cent) * (fresh - cent)).reshape(-1).tolist():
            shift = shift + v
        cent = fresh
        n_iter = it + 1
        if old is not None and np.array_equal(labels, old):
            reason = STRICT
            break
        if shift <= ta:
            reason = TOL
            break
        old = labels
    if reason != STRICT:
        labels, best, gap = assign(X, cent)
        if gaps is not None:
            gaps.append(float(gap.min()))
    own = distances_to_labels(X, cent, labels)
    inertia = 0.0
    for v in own.tolist():
        inertia = inertia + v
    return cent, labels, dict(n_iter=n_iter, stop_reason=reason, inertia=inertia, relocations=relocations, tol_abs=ta)


def distances_to_labels(X, cent, labels):
    Xf = np.asarray(X, np.float64)
    c = np.asarray(cent, np.float64)[np.asarray(labels, np.int64)]
    acc = np.zeros(Xf.shape[0], np.float64)
    for d in range(Xf.shape[1]):
        t = Xf[:, d] - c[:, d]
        acc = acc + t * t
    return acc


def sort_by_energy(centroids, labels):
    """VQ.py:87-100 with energy = the sum of squares in float64 (A14)."""
    K = centroids.shape[0]
    e = np.array([np.sum(np.asarray(c, np.float64) * np.asarray(c, np.float64)) for c in centroids])
    order = np.argsort(e)
    lut = np.empty_like(order, dtype=np.int16)
    lut[order] = np.arange(K)
    out = np.empty_like(centroids)
    for i in range(K):
        out[lut[i]] = centroids[i]
    return out, lut[labels]


def decode(labels, centroids, BS, C):
    """VQ.py:117-137 and .astype(np.uint8): labels (Hl, Wl), centroids (K, BS*BS*C) -> u8 image."""
    Hl, Wl = labels.shape
    c = np.asarray(centroids, np.float64).reshape(centroids.shape[0], BS, BS, C)
    y = np.empty((Hl * BS, Wl * BS, C), np.int16)
    for by in range(Hl):
        for bx in range(Wl):
            y[by * BS:(by + 1) * BS, bx * BS:(bx + 1) * BS, :] = c[labels[by, bx]]
    return y.astype(np.uint8)


def vq_encode(img, BS, K, seed=0):
    """VQ.CoDec.quantize over the restated fit: (labels (H/BS, W/BS) uint16, codebook (K, BS*BS, C) float64)."""
    X = blocks(img, BS)
    K = min(K, X.shape[0])
    cent, labels, rep = fit(X, K, seed)
    cent, labels = sort_by_energy(cent, labels)
    H, W, C = img.shape
    return labels.reshape(H // BS, W // BS).astype(np.uint16), cent.reshape(K, BS * BS, C), rep


def color_vq_encode(img, K, seed=0):
    """color-VQ.CoDec.quantize over the restated fit: (labels (H, W) uint16, codebook (K, 3) uint8)."""
    X = blocks(img, 1)
    cent, labels, rep = fit(X, K, seed)
    return labels.reshape(img.shape[:2]).astype(np.uint16), cent.astype(np.uint8), rep

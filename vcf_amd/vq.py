"""The vector quantizer on the GPU (src/VQ.py, src/color-VQ.py; vcf_vq.hip).

k-means as sklearn.cluster.KMeans(algorithm="lloyd", n_init=1) runs it, on
the BS x BS x C blocks of one u8 frame: assign (the nearest centroid of every
block, float64), accumulate (integer sums and counts per cluster), init_pp
(k-means++ in exact integers, from a seed), fit (the Lloyd loop) and decode
(labels and codebook back to pixels).  The *_device functions take and return
DeviceBuffers; the others are host conveniences.  There is no CPU path: the
arithmetic runs in libvcf_amd.so and is stated in include/vcf_amd.h.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import call
from .device import DeviceBuffer, _h

STOP_STRICT, STOP_TOL, STOP_MAX_ITER = 0, 1, 2
STOP_NAMES = {STOP_STRICT: "strict", STOP_TOL: "tol", STOP_MAX_ITER: "max_iter"}
DEFAULT_MAX_ITER = 300        # sklearn.cluster.KMeans
DEFAULT_TOL = 1e-4
MAX_K = 4096


class _Report(ctypes.Structure):
    """vcf_vq_report (include/vcf_amd.h)."""
    _fields_ = [("n_iter", ctypes.c_int32), ("stop_reason", ctypes.c_int32), ("relocations", ctypes.c_int64),
                ("inertia", ctypes.c_double), ("tol_abs", ctypes.c_double)]


@dataclass
class FitReport:
    n_iter: int
    stop_reason: str        # "strict", "tol" or "max_iter"
    inertia: float
    relocations: int
    tol_abs: float


def _frame(img: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(img)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3:
        raise ValueError("img must be H x W x C")
    if a.dtype != np.uint8:
        raise TypeError("img must be uint8")
    return a


def shape_of(H: int, W: int, C: int, BS: int):
    """(N vectors, D values each); the library itself refuses a frame that is no whole number of blocks."""
    BS = int(BS)
    if BS < 1:
        return 0, 0
    return (H // BS) * (W // BS), BS * BS * C


# ---- device arrays ---------------------------------------------------------------
def assign_device(img: DeviceBuffer, H, W, C, BS, cent: DeviceBuffer, K, labels: DeviceBuffer,
                  dist: DeviceBuffer | None = None, stream=None) -> None:
    call("vcf_vq_assign", img.ptr, int(H), int(W), int(C), int(BS), cent.ptr, int(K), labels.ptr,
         dist.ptr if dist is not None else None, _h(stream))


def accumulate_device(img: DeviceBuffer, H, W, C, BS, labels: DeviceBuffer, K, sums: DeviceBuffer,
                      counts: DeviceBuffer, stream=None) -> None:
    call("vcf_vq_accumulate", img.ptr, int(H), int(W), int(C), int(BS), labels.ptr, int(K), sums.ptr, counts.ptr,
         _h(stream))


def init_pp_device(img: DeviceBuffer, H, W, C, BS, K, seed, cent: DeviceBuffer, stream=None) -> np.ndarray:
    """k-means++ into `cent`; returns the K chosen vector indices.  Synchronises the stream."""
    ids = np.empty(max(int(K), 1), np.int64)
    call("vcf_vq_init_pp", img.ptr, int(H), int(W), int(C), int(BS), int(K), int(seed) & (2 ** 64 - 1), cent.ptr,
         ids.ctypes.data_as(ctypes.c_void_p), _h(stream))
    return ids[:int(K)]


def fit_device(img: DeviceBuffer, H, W, C, BS, K, cent: DeviceBuffer, labels: DeviceBuffer, seed=0,
               max_iter=DEFAULT_MAX_ITER, tol=DEFAULT_TOL, init: DeviceBuffer | None = None, stream=None) -> FitReport:
    """The Lloyd loop into `cent` and `labels`, from `init` or k-means++(seed).  Synchronises the stream."""
    rep = _Report()
    call("vcf_vq_fit", img.ptr, int(H), int(W), int(C), int(BS), int(K), int(seed) & (2 ** 64 - 1), int(max_iter),
         float(tol), init.ptr if init is not None else None, cent.ptr, labels.ptr, ctypes.byref(rep), _h(stream))
    return FitReport(rep.n_iter, STOP_NAMES[rep.stop_reason], rep.inertia, rep.relocations, rep.tol_abs)


def decode_device(labels: DeviceBuffer, Hl, Wl, C, BS, cent: DeviceBuffer, K, out: DeviceBuffer, stream=None) -> None:
    """Raises IndexError for a label >= K, as indexing the codebook does in numpy."""
    bad = DeviceBuffer(4)
    try:
        bad.fill(0, stream)
        call("vcf_vq_decode", labels.ptr, int(Hl), int(Wl), int(C), int(BS), cent.ptr, int(K), out.ptr, bad.ptr,
             _h(stream))
        flag = bad.download(np.zeros(1, np.int32), stream)
        if stream is not None:
            stream.synchronize()
        if flag[0]:
            raise IndexError(f"label out of bounds for the {int(K)} centroids")
    finally:
        bad.free()


# ---- host arrays -----------------------------------------------------------------
def _free(*bufs):
    for b in bufs:
        if b is not None:
            b.free()


def _cent(centroids, D) -> np.ndarray:
    c = np.ascontiguousarray(centroids, dtype=np.float64)
    c = c.reshape(c.shape[0], -1)
    if c.shape[1] != D:
        raise ValueError(f"centroids of {c.shape[1]} values for vectors of {D}")
    return c


def assign(img: np.ndarray, BS: int, centroids, want_dist: bool = False):
    """labels (N,) uint16 [, squared distances (N,) float64] of the blocks of img."""
    a = _frame(img)
    H, W, C = a.shape
    N, D = shape_of(H, W, C, BS)
    c = _cent(centroids, D) if D else np.zeros((1, 1))
    dimg = dc = dl = dd = None
    try:
        dimg, dc = DeviceBuffer.from_array(a), DeviceBuffer.from_array(c)
        dl = DeviceBuffer(N * 2)
        dd = DeviceBuffer(N * 8) if want_dist else None
        assign_device(dimg, H, W, C, BS, dc, c.shape[0], dl, dd)
        labels = dl.download(np.empty(N, np.uint16))
        return (labels, dd.download(np.empty(N, np.float64))) if want_dist else labels
    finally:
        _free(dimg, dc, dl, dd)


def accumulate(img: np.ndarray, BS: int, labels, K: int):
    """(sums (K, D) int64, counts (K,) int64) of the blocks of img under `labels`."""
    a = _frame(img)
    H, W, C = a.shape
    N, D = shape_of(H, W, C, BS)
    lab = np.ascontiguousarray(labels, dtype=np.uint16).reshape(-1)
    if lab.size != N:
        raise ValueError(f"{lab.size} labels for {N} vectors")
    K = int(K)
    dimg = dl = ds = dn = None
    try:
        dimg, dl = DeviceBuffer.from_array(a), DeviceBuffer.from_array(lab)
        ds, dn = DeviceBuffer(max(K, 1) * max(D, 1) * 8), DeviceBuffer(max(K, 1) * 8)
        accumulate_device(dimg, H, W, C, BS, dl, K, ds, dn)
        return ds.download(np.empty((K, D), np.int64)), dn.download(np.empty(K, np.int64))
    finally:
        _free(dimg, dl, ds, dn)


def init_pp(img: np.ndarray, BS: int, K: int, seed: int = 0):
    """k-means++: (centroids (K, D) float64, the chosen vector indices (K,) int64)."""
    a = _frame(img)
    H, W, C = a.shape
    N, D = shape_of(H, W, C, BS)
    K = int(K)
    dimg = dc = None
    try:
        dimg, dc = DeviceBuffer.from_array(a), DeviceBuffer(max(K, 1) * max(D, 1) * 8)
        ids = init_pp_device(dimg, H, W, C, BS, K, seed, dc)
        return dc.download(np.empty((K, D), np.float64)), ids
    finally:
        _free(dimg, dc)


def fit(img: np.ndarray, BS: int, K: int, seed: int = 0, max_iter: int = DEFAULT_MAX_ITER, tol: float = DEFAULT_TOL,
        init=None):
    """KMeans(n_clusters=K, n_init=1, algorithm="lloyd").fit(blocks):
    (centroids (K, D) float64, labels (N,) uint16, FitReport)."""
    a = _frame(img)
    H, W, C = a.shape
    N, D = shape_of(H, W, C, BS)
    K = int(K)
    dimg = dc = dl = di = None
    try:
        dimg = DeviceBuffer.from_array(a)
        dc, dl = DeviceBuffer(max(K, 1) * max(D, 1) * 8), DeviceBuffer(N * 2)
        if init is not None:
            c0 = _cent(init, D)
            if c0.shape[0] != K:
                raise ValueError(f"{c0.shape[0]} initial centroids for K = {K}")
            di = DeviceBuffer.from_array(c0)
        rep = fit_device(dimg, H, W, C, BS, K, dc, dl, seed, max_iter, tol, di)
        return dc.download(np.empty((K, D), np.float64)), dl.download(np.empty(N, np.uint16)), rep
    finally:
        _free(dimg, dc, dl, di)


def decode(labels: np.ndarray, centroids, BS: int, C: int) -> np.ndarray:
    """labels (Hl, Wl) and the codebook -> the u8 image (Hl*BS, Wl*BS, C)."""
    lab = np.ascontiguousarray(labels)
    if lab.ndim != 2:
        raise ValueError(f"labels of shape {lab.shape}: expected Hl x Wl")
    if lab.dtype != np.uint16:
        raise TypeError("labels must be uint16")
    Hl, Wl = lab.shape
    BS, C = int(BS), int(C)
    c = _cent(centroids, BS * BS * C)
    out = np.empty((Hl * BS, Wl * BS, C), np.uint8)
    dl = dc = do = None
    try:
        dl, dc, do = DeviceBuffer.from_array(lab), DeviceBuffer.from_array(c), DeviceBuffer(out.nbytes)
        decode_device(dl, Hl, Wl, C, BS, dc, c.shape[0], do)
        return do.download(out)
    finally:
        _free(dl, dc, do)

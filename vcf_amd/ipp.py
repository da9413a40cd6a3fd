"""IPP temporal tools on the GPU (src/IPP_DCT.py): block matching, motion
compensation, residual and reconstruction through libvcf_amd.so.  Host
arrays in and out (the IPP driver keeps a GOP's frames on the device when it
calls the C ABI directly)."""
from __future__ import annotations

import numpy as np

from . import _lib as L
from .device import DeviceBuffer


def _rgb(a):
    a = np.ascontiguousarray(a)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError("expected H x W x 3 uint8")
    return a


def _check_subpel(subpel) -> int:
    if subpel not in (1, 2, 4):
        raise ValueError(f"subpel {subpel!r}: 1 (whole), 2 (half) or 4 (quarter pel)")
    return int(subpel)


MAX_LEVELS = 3


def check_levels(levels, bs, fast=False) -> int:
    """The levels of the hierarchical search (include/vcf_amd.h): 0 .. 3, with bs a multiple of
    2^levels and bs >> levels >= 2, and not with the three-step search."""
    if isinstance(levels, bool) or levels not in range(MAX_LEVELS + 1):
        raise ValueError(f"levels {levels!r}: 0 .. {MAX_LEVELS}")
    levels = int(levels)
    if levels and (int(bs) % (1 << levels) or (int(bs) >> levels) < 2):
        raise ValueError(f"block size {bs} with {levels} levels: a multiple of {1 << levels}, at least {2 << levels}")
    if levels and fast:
        raise ValueError("the three-step search (fast) is a whole-frame tool: not with levels > 0")
    return levels


def hier_workspace_bytes(H: int, W: int, levels: int) -> int:
    """vcf_ipp_hier_workspace_bytes: the two gray planes and both pyramids."""
    import ctypes
    n = ctypes.c_int64(0)
    L.call("vcf_ipp_hier_workspace_bytes", int(H), int(W), int(levels), ctypes.byref(n))
    return int(n.value)


def block_matching(ref: np.ndarray, cur: np.ndarray, bs: int = 16, sr: int = 8, fast: bool = False,
                   variant: int = 0, subpel: int = 1, levels: int = 0) -> np.ndarray:
    """IPP.block_matching (IPP_DCT.py:344-376) -> (H//bs, W//bs, 2) float32 (dx, dy).
    variant 0: word kernels (full search for bs % 4 == 0, parallel-round TSS for bs 16; the product's rule),
    1: byte / serial kernels (the A/B library's twin; same vectors).
    subpel 2 / 4: the integer search refined to half / quarter pel (vcf_ipp_block_match_subpel;
    not in the reference), vectors in multiples of 1/subpel.
    levels 1 .. 3: the coarse-to-fine search on a luma pyramid (vcf_ipp_block_match_hier; not in the
    reference), sr applied at the top level: vectors within +-(sr 2^levels + 2^levels - 1)."""
    ref, cur = _rgb(ref), _rgb(cur)
    subpel = _check_subpel(subpel)
    levels = check_levels(levels, bs, fast)
    if levels and variant != 0:
        raise ValueError("the hierarchical search runs the product's integer kernels (variant 0)")
    if subpel > 1 and variant != 0:
        raise ValueError("the sub-pel search runs after the product's integer kernels (variant 0)")
    H, W = ref.shape[:2]
    mv = np.zeros((H // bs, W // bs, 2), np.float32)
    if mv.size == 0:
        return mv
    dr, dc = DeviceBuffer.from_array(ref), DeviceBuffer.from_array(cur)
    nws = hier_workspace_bytes(H, W, levels) if levels else 2 * H * W
    dm, dg = DeviceBuffer(mv.nbytes), DeviceBuffer(nws)
    try:
        if levels:
            L.call("vcf_ipp_block_match_hier", dr.ptr, dc.ptr, H, W, int(bs), int(sr), levels, subpel, dm.ptr, dg.ptr,
                   nws, None)
        elif subpel > 1:
            L.call("vcf_ipp_block_match_subpel", dr.ptr, dc.ptr, H, W, int(bs), int(sr), int(bool(fast)), subpel,
                   dm.ptr, dg.ptr, None)
        else:
            L.call_v(int(variant), "vcf_ipp_block_match", dr.ptr, dc.ptr, H, W, int(bs), int(sr), int(bool(fast)),
                     dm.ptr, dg.ptr, None)
        return dm.download(mv)
    finally:
        for b in (dr, dc, dm, dg):
            b.free()


OBMC_BLOCK_SIZES = (4, 8, 16, 32, 64)


def check_obmc_bs(bs) -> int:
    """The block sides of the overlapped compensator (include/vcf_amd.h)."""
    if isinstance(bs, bool) or bs not in OBMC_BLOCK_SIZES:
        raise ValueError(f"block size {bs!r} with obmc: 4, 8, 16, 32 or 64")
    return int(bs)


def mc_entry(subpel: int = 1, obmc: bool = False) -> str:
    """The compensator of the C ABI for a precision and the obmc switch (one signature for all three)."""
    if obmc:
        return "vcf_ipp_motion_compensate_obmc"
    return "vcf_ipp_motion_compensate_qpel" if subpel > 1 else "vcf_ipp_motion_compensate"


def motion_compensate(frame: np.ndarray, mv: np.ndarray, bs: int = 16, subpel: int = 1, obmc: bool = False) -> np.ndarray:
    """IPP.motion_compensate (IPP_DCT.py:378-395); subpel > 1: the bilinear quarter-pel
    compensator (vcf_ipp_motion_compensate_qpel), which rounds the field to quarter pels.
    obmc: the overlapped compensator (vcf_ipp_motion_compensate_obmc; not in the reference) for
    every subpel (a whole-pel field has zero fractions); bs must be 4, 8, 16, 32 or 64."""
    frame = _rgb(frame)
    name = mc_entry(_check_subpel(subpel), obmc)
    if obmc:
        bs = check_obmc_bs(bs)
    H, W = frame.shape[:2]
    mv = np.ascontiguousarray(mv, np.float32)
    if mv.shape != (H // bs, W // bs, 2):
        raise ValueError(f"motion field shape {mv.shape} != {(H // bs, W // bs, 2)}")
    out = np.empty_like(frame)
    df, dm, do = DeviceBuffer.from_array(frame), DeviceBuffer.from_array(mv if mv.size else np.zeros(2, np.float32)), \
        DeviceBuffer(frame.nbytes)
    try:
        L.call(name, df.ptr, dm.ptr, H, W, int(bs), do.ptr, None)
        return do.download(out)
    finally:
        for b in (df, dm, do):
            b.free()


def _binary(name, a, b):
    a, b = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
    if a.shape != b.shape:
        raise ValueError("shape mismatch")
    out = np.empty_like(a)
    if a.size == 0:
        return out
    da, db, do = DeviceBuffer.from_array(a), DeviceBuffer.from_array(b), DeviceBuffer(a.nbytes)
    try:
        L.call(name, da.ptr, db.ptr, a.size, do.ptr, None)
        return do.download(out)
    finally:
        for x in (da, db, do):
            x.free()


def residual(cur: np.ndarray, comp: np.ndarray) -> np.ndarray:
    """clip(cur - comp + 128, 0, 255) as uint8 (IPP_DCT.py:547-551)."""
    return _binary("vcf_ipp_residual", cur, comp)


def reconstruct(comp: np.ndarray, rec: np.ndarray) -> np.ndarray:
    """clip(comp + rec - 128, 0, 255) as uint8 (IPP_DCT.py:559-561)."""
    return _binary("vcf_ipp_reconstruct", comp, rec)


def rdo_modes(cur: np.ndarray, comp: np.ndarray, bs: int = 16, Q: int = 32, lam: float = 0.0,
              with_costs: bool = False):
    """-R block modes (IPP_DCT.py:441-468 + rdo_block_decision :290-342): (H//bs, W//bs) u8, 1 = I, 0 = P."""
    cur, comp = _rgb(cur), _rgb(comp)
    if cur.shape != comp.shape:
        raise ValueError("shape mismatch")
    H, W = cur.shape[:2]
    modes = np.zeros((H // bs, W // bs), np.uint8)
    costs = np.zeros((H // bs, W // bs, 4), np.float64)
    if modes.size == 0:
        return (modes, costs) if with_costs else modes
    dc, dp = DeviceBuffer.from_array(cur), DeviceBuffer.from_array(comp)
    dm, dk = DeviceBuffer(modes.nbytes), DeviceBuffer(costs.nbytes)
    try:
        L.call("vcf_ipp_rdo_modes", dc.ptr, dp.ptr, H, W, int(bs), int(Q), float(lam), dm.ptr, dk.ptr, None)
        dm.download(modes)
        dk.download(costs)
        return (modes, costs) if with_costs else modes
    finally:
        for b in (dc, dp, dm, dk):
            b.free()


def _modal(name, a, b, modes, bs):
    a, b = _rgb(a), _rgb(b)
    if a.shape != b.shape:
        raise ValueError("shape mismatch")
    H, W = a.shape[:2]
    m = np.ascontiguousarray(modes, np.uint8)
    if m.shape != (H // bs, W // bs):
        raise ValueError(f"mode map shape {m.shape} != {(H // bs, W // bs)}")
    out = np.empty_like(a)
    da, db, do = DeviceBuffer.from_array(a), DeviceBuffer.from_array(b), DeviceBuffer(a.nbytes)
    dm = DeviceBuffer.from_array(m if m.size else np.zeros(1, np.uint8))
    try:
        L.call(name, da.ptr, db.ptr, dm.ptr, H, W, int(bs), do.ptr, None)
        return do.download(out)
    finally:
        for x in (da, db, do, dm):
            x.free()


def rdo_residual(cur: np.ndarray, comp: np.ndarray, modes: np.ndarray, bs: int = 16) -> np.ndarray:
    """frame_to_encode_shifted (IPP_DCT.py:489-505)."""
    return _modal("vcf_ipp_rdo_residual", cur, comp, modes, bs)


def rdo_reconstruct(comp: np.ndarray, rec: np.ndarray, modes: np.ndarray, bs: int = 16) -> np.ndarray:
    """Mode-aware P-frame reconstruction (IPP_DCT.py:512-526, 770-790)."""
    return _modal("vcf_ipp_rdo_reconstruct", comp, rec, modes, bs)


def _check_bs(bs) -> int:
    if not 1 <= int(bs) <= 64:
        raise ValueError(f"block size {bs!r}: 1 .. 64")
    return int(bs)


def bipred_residual(cur: np.ndarray, cf: np.ndarray, cb: np.ndarray, bs: int = 16):
    """B-frame decision and residual (vcf_ipp_bipred_residual; not in the reference): per full
    block the argmin of (SAD, mode) over cf, cb and (cf + cb + 1) >> 1 -> ((H//bs, W//bs) u8
    modes, clip(cur - pred + 128) over the whole frame, pred = 0 outside the full blocks)."""
    cur, cf, cb = _rgb(cur), _rgb(cf), _rgb(cb)
    bs = _check_bs(bs)
    if not cur.shape == cf.shape == cb.shape:
        raise ValueError("shape mismatch")
    H, W = cur.shape[:2]
    modes, res = np.zeros((H // bs, W // bs), np.uint8), np.empty_like(cur)
    if res.size == 0:
        return modes, res
    dc, df, db = (DeviceBuffer.from_array(a) for a in (cur, cf, cb))
    dm, do = DeviceBuffer(max(1, modes.nbytes)), DeviceBuffer(res.nbytes)
    try:
        L.call("vcf_ipp_bipred_residual", dc.ptr, df.ptr, db.ptr, H, W, bs, dm.ptr, do.ptr, None)
        if modes.size:
            dm.download(modes)
        return modes, do.download(res)
    finally:
        for x in (dc, df, db, dm, do):
            x.free()


def bipred_reconstruct(cf: np.ndarray, cb: np.ndarray, modes: np.ndarray, rec: np.ndarray, bs: int = 16) -> np.ndarray:
    """B-frame reconstruction (vcf_ipp_bipred_reconstruct): pred from the mode map (0 cf, 1 cb,
    2 their rounded average; 0 outside the full blocks), then clip(pred + rec - 128)."""
    cf, cb, rec = _rgb(cf), _rgb(cb), _rgb(rec)
    bs = _check_bs(bs)
    if not cf.shape == cb.shape == rec.shape:
        raise ValueError("shape mismatch")
    H, W = cf.shape[:2]
    m = np.asarray(modes)
    if m.dtype != np.uint8 or m.shape != (H // bs, W // bs):
        raise ValueError(f"mode map {m.dtype} {m.shape} != uint8 {(H // bs, W // bs)}")
    if m.size and int(m.max()) > 2:
        raise ValueError(f"B-frame mode {int(m.max())}: 0 (forward), 1 (backward) or 2 (average)")
    m = np.ascontiguousarray(m)
    out = np.empty_like(cf)
    if out.size == 0:
        return out
    df, db, dr, do = DeviceBuffer.from_array(cf), DeviceBuffer.from_array(cb), DeviceBuffer.from_array(rec), \
        DeviceBuffer(out.nbytes)
    dm = DeviceBuffer.from_array(m if m.size else np.zeros(1, np.uint8))
    try:
        L.call("vcf_ipp_bipred_reconstruct", df.ptr, db.ptr, dm.ptr, dr.ptr, H, W, bs, do.ptr, None)
        return do.download(out)
    finally:
        for x in (df, db, dr, do, dm):
            x.free()


def check_mv_refine(lam, iterations):
    """The limits of vcf_ipp_mv_refine (include/vcf_amd.h): lambda 0 .. 1024, 1 .. 4 iterations."""
    if isinstance(lam, bool) or not isinstance(lam, (int, np.integer)) or not 0 <= lam <= 1024:
        raise ValueError(f"mv lambda {lam!r}: an integer 0 .. 1024")
    if isinstance(iterations, bool) or iterations not in (1, 2, 3, 4):
        raise ValueError(f"mv iterations {iterations!r}: 1 .. 4")
    return int(lam), int(iterations)


def mv_refine_workspace_bytes(H: int, W: int, bs: int) -> int:
    """vcf_ipp_mv_refine_workspace_bytes: the two gray planes and a second field."""
    import ctypes
    n = ctypes.c_int64(0)
    L.call("vcf_ipp_mv_refine_workspace_bytes", int(H), int(W), int(bs), ctypes.byref(n))
    return int(n.value)


def refine_field(ref: np.ndarray, cur: np.ndarray, mv: np.ndarray, bs: int, subpel: int = 1, lam: int = 0,
                 iterations: int = 2) -> np.ndarray:
    """vcf_ipp_mv_refine (not in the reference): every block re-decides its vector among its own, the
    motion coder's predictor, its four neighbours' and zero by SAD + lam * bits -> the new field."""
    ref, cur = _rgb(ref), _rgb(cur)
    if ref.shape != cur.shape:
        raise ValueError("shape mismatch")
    subpel = _check_subpel(subpel)
    lam, iterations = check_mv_refine(lam, iterations)
    bs = _check_bs(bs)
    H, W = ref.shape[:2]
    mv = np.ascontiguousarray(mv, np.float32)
    if mv.shape != (H // bs, W // bs, 2):
        raise ValueError(f"motion field shape {mv.shape} != {(H // bs, W // bs, 2)}")
    if mv.size == 0:
        return mv.copy()
    nws = mv_refine_workspace_bytes(H, W, bs)
    dr, dc, dm, dw = DeviceBuffer.from_array(ref), DeviceBuffer.from_array(cur), DeviceBuffer.from_array(mv), \
        DeviceBuffer(nws)
    try:
        L.call("vcf_ipp_mv_refine", dr.ptr, dc.ptr, H, W, bs, subpel, lam, iterations, dm.ptr, dw.ptr, nws, None)
        return dm.download(np.empty_like(mv))
    finally:
        for b in (dr, dc, dm, dw):
            b.free()


def _field_q(q) -> np.ndarray:
    q = np.asarray(q)
    if q.ndim != 3 or q.shape[2] != 2 or q.dtype.kind not in "iu":
        raise ValueError("expected an nby x nbx x 2 integer field (quarter pels)")
    if q.size and int(np.abs(q.astype(np.int64)).max()) > 1 << 15:
        raise ValueError("vector component beyond +-2^15 quarter pels")
    return np.ascontiguousarray(q, np.int32)


def mv_encode(q: np.ndarray, step: int = 1) -> bytes:
    """vcf_mv_encode (host code): an nby x nbx x 2 integer field of quarter-pel vectors on the step
    grid (step = 4 / subpel) -> median-predicted signed exp-Golomb codes."""
    import ctypes
    q = _field_q(q)
    nby, nbx = q.shape[:2]
    cap = ctypes.c_int64(0)
    L.call("vcf_mv_encode_bound", nby, nbx, ctypes.byref(cap))
    out, n = np.empty(max(1, cap.value), np.uint8), ctypes.c_int64(0)
    L.call("vcf_mv_encode", q.ctypes.data if q.size else out.ctypes.data, nby, nbx, int(step), out.ctypes.data,
           cap.value, ctypes.byref(n))
    return out[:n.value].tobytes()


def mv_decode(data: bytes, nby: int, nbx: int, step: int = 1) -> np.ndarray:
    """vcf_mv_decode: the inverse -> (nby, nbx, 2) int32; ValueError for a stream the encoder does not write."""
    if nby < 0 or nbx < 0:
        raise ValueError(f"motion field of {nby} x {nbx} blocks")
    buf = np.frombuffer(bytes(data), np.uint8)
    src = buf if buf.size else np.zeros(1, np.uint8)
    q = np.zeros((int(nby), int(nbx), 2), np.int32)
    L.call("vcf_mv_decode", src.ctypes.data, buf.size, int(nby), int(nbx), int(step),
           q.ctypes.data if q.size else src.ctypes.data)
    return q

"""IPP hybrid video coding: the drop-in for src/IPP_DCT.py (IPP + CoDec).

Each GOP is an I-frame coded by the spatial codec (--st: 2D-DCT, the
default, or 2D-DWT -- the reference subclasses whichever module --st names,
IPP_DCT.py:45-87; here codec_class(st) picks CoDec or CoDecDWT)
followed by P-frames: block matching against the previous reconstruction,
motion compensation, the residual shifted by 128 and clipped, coded by the
same spatial codec, and the reconstruction clip(pred + rec - 128)
(IPP_DCT.py:397-575).  Files are the reference's: {prefix}_O_%04d.png
(originals), {prefix}_{I,P}_{n}_enc.tif + _shape.bin, {prefix}_mv.npz,
{prefix}_meta.json; decode writes {out}_%04d.png.

Block matching, compensation, residual and reconstruction run on the GPU
(vcf_amd/csrc/vcf_ipp.hip); the spatial codec is the 2D-DCT CoDec (GPU).
encode_decode_proxy (:595-626) round-trips through temporary PNG files in
the reference; here the coded frame is decoded from the same code-stream in
memory (PNG is lossless, so the reconstruction is identical).

GOPs are independent, so they shard over ranks (one process per GPU); the
per-frame sizes and motion fields are gathered on rank 0, which writes the
metadata (at most ceil(N/G) ranks are busy).
-R/--rdo_lambda > 0 runs the block-level mode decision on the GPU
(vcf_amd/csrc/vcf_ipp_rdo.hip: rdo_block_decision :290-342 per block, the
mixed-mode frame :489-505 and its reconstruction :512-526); the motion file
then also carries each P frame's mode map, like the reference's
{"mv", "modes"} entries, and the decoder reconstructs mode by mode
(:770-790).
--subpel 2 / 4 (not in the reference) refines the vectors to half / quarter
pel and predicts by bilinear interpolation (vcf_amd/csrc/vcf_ipp_subpel.hip);
meta.json then carries "subpel" and the decoder interpolates alike.
--bframes N (not in the reference) puts N bidirectionally predicted frames
between two anchors (gop_types): an anchor predicts from the anchor before it,
a B-frame from both anchors around it, block by block from the past one, the
future one or their average (vcf_amd/csrc/vcf_ipp_bipred.hip), and nothing
predicts from a B-frame.  The B-frames go to {prefix}_B_{n}_enc files, their
fields and mode maps to "bmv_f32" / "bmodes_u8" of the motion file, and
meta.json carries "bframes", "frame_types" and "B_info".
--me_levels L (not in the reference) makes every motion search coarse to fine
on a luma pyramid (vcf_amd/csrc/vcf_ipp_hier.hip): -S applies on level L and
the vectors reach +-(S 2^L + 2^L - 1).  It changes only the vectors chosen: no
file, array or meta.json key is added, and the decoder does not know of it.
--obmc (not in the reference) replaces every motion compensation, the B-frames'
two included, by the overlapped one (vcf_amd/csrc/vcf_ipp_obmc.hip): a pixel is
blended from its own block's vector and its nearest neighbours'.  -M must be 4,
8, 16, 32 or 64; the searches, the motion file and the file names do not change;
meta.json carries "obmc": true and the decoder compensates alike.
--mvc (not in the reference) writes the motion file as {prefix}_mv.vmv instead
of _mv.npz (vcf_amd/codec/mvfile.py): every field predicted from its neighbours
by a median and coded with signed exp-Golomb codes (vcf_amd/csrc/vcf_mvc.cpp),
the mode maps as one zlib stream; meta.json carries "mv_codec": "median-eg0" and
the decoder dispatches on it.
--mv_lambda L > 0 (not in the reference) re-decides every block's vector after
every search by SAD + L * (that coder's bits), --mv_iters passes
(vcf_amd/csrc/vcf_ipp_mvrefine.hip).  It changes only the vectors chosen; the
decoder does not know of it.
"""
from __future__ import annotations

import glob
import io
import json
import logging
import os
import struct

import numpy as np

from .. import ipp as K
from ..ipp import check_levels, check_mv_refine, check_obmc_bs, hier_workspace_bytes, mc_entry, mv_refine_workspace_bytes
from . import mvfile, shard
from .dct2d import CoDec as DCTCoDec
from .dwt2d import CoDec as DWTCoDec
from .eic import read_image, write_image

_TMP_DIR = "/tmp"   # os.path.join(_SCRIPT_DIR, "/tmp") == "/tmp" (IPP_DCT.py:20)


def resolve_prefix(prefix: str) -> str:
    """IPP_DCT.py:132-142."""
    if prefix.startswith("./"):
        return os.path.join(_TMP_DIR, prefix[2:])
    if not os.path.isabs(prefix):
        return os.path.join(_TMP_DIR, prefix)
    return prefix


def _ensure_dir(prefix: str):
    d = os.path.dirname(prefix)
    if d:
        os.makedirs(d, exist_ok=True)


def read_frames(src: str, n: int):
    """The encoder's input: a video (needs PyAV, absent here), a printf
    pattern of PNGs, a directory of PNGs or an .npy (N x H x W x 3)."""
    if src.endswith(".npy"):
        return list(np.load(src, allow_pickle=False)[:n])
    if "%" in src:
        files = [src % i for i in range(n)]
    elif os.path.isdir(src):
        files = sorted(glob.glob(os.path.join(src, "*.png")))[:n]
    else:
        try:
            import av
        except ImportError as e:
            raise NotImplementedError(f"{src}: video demux needs PyAV, which is not installed; pass a PNG "
                                      f"pattern, a directory of PNGs or an .npy of frames") from e
        frames = []
        with av.open(src) as c:
            for fr in c.decode(video=0):
                frames.append(np.array(fr.to_image().convert("RGB")))
                if len(frames) >= n:
                    break
        return frames
    return [read_image(f)[0] for f in files]


MAX_BFRAMES = 7


def gop_types(L: int, N: int) -> str:
    """Display-order frame types of a GOP of L frames with N B-frames between two anchors:
    I first, anchors every N + 1 frames and at the last frame, B strictly between anchors."""
    if L < 1 or not 0 <= N <= MAX_BFRAMES:
        raise ValueError(f"gop_types({L}, {N}): L >= 1 and 0 <= N <= {MAX_BFRAMES}")
    t, a = ["B"] * L, 0
    t[0] = "I"
    while a < L - 1:
        a = min(a + N + 1, L - 1)
        t[a] = "P"
    return "".join(t)


def sequence_types(n_frames: int, gop_size: int, N: int) -> str:
    """gop_types of every GOP of the sequence, in display order."""
    return "".join(gop_types(min(gop_size, n_frames - g0), N) for g0 in range(0, n_frames, gop_size))


def _anchor_intervals(types: str):
    """(past anchor, closing anchor) positions of a GOP, in coding order."""
    anchors = [i for i, t in enumerate(types) if t != "B"]
    return list(zip(anchors, anchors[1:]))


class _IPP:
    """IPP_DCT.CoDec (:578-720) over a spatial codec base class (the MRO's next)."""

    def __init__(self, args, group=None):
        if getattr(args, "filter", "no_filter") == "deblock":
            raise NotImplementedError("filter 'deblock' with IPP: the filter would sit inside the prediction loop "
                                      "and change the frames the encoder predicted from")
        super().__init__(args)
        if getattr(self, "lm", None) is not None:
            # the GOP loop keeps indices in HBM through the fused deadzone kernels
            raise NotImplementedError("IPP with -a LloydMax: only deadzone is on the HIP path")
        self.gop_size = getattr(args, "gop_size", 10) or 10
        self.block_size_ME = getattr(args, "block_size_ME", 16) or 16
        self.search_range = getattr(args, "search_range", 8)
        if self.search_range is None:
            self.search_range = 8
        self.use_fast = bool(getattr(args, "fast", False))
        self.rdo_lambda = float(getattr(args, "rdo_lambda", 0.0) or 0.0)
        # motion precision (not in the reference): 1 whole, 2 half, 4 quarter pel; the decoder takes it from meta.json
        self.subpel = int(getattr(args, "subpel", 1) or 1)
        if self.subpel not in (1, 2, 4):
            raise ValueError(f"--subpel {self.subpel}: 1, 2 or 4")
        # B-frames between two anchors (not in the reference); the decoder takes the structure from meta.json
        self.bframes = int(getattr(args, "bframes", 0) or 0)
        if not 0 <= self.bframes <= MAX_BFRAMES:
            raise ValueError(f"--bframes {self.bframes}: 0 .. {MAX_BFRAMES}")
        if self.bframes and self.rdo_lambda > 0:
            raise NotImplementedError("--bframes with -R: no mode-decision anchors beside B-frames yet")
        # levels of the hierarchical motion search (not in the reference); the encoder's choice alone
        self.me_levels = check_levels(int(getattr(args, "me_levels", 0) or 0), self.block_size_ME, self.use_fast)
        # overlapped block motion compensation (not in the reference); the decoder takes it from meta.json
        self.obmc = bool(getattr(args, "obmc", False))
        if self.obmc:
            try:
                check_obmc_bs(self.block_size_ME)
            except ValueError:
                raise ValueError(f"--obmc with -M {self.block_size_ME}: -M must be 4, 8, 16, 32 or 64") from None
        # the coded motion file (not in the reference); the decoder takes it from meta.json
        self.mvc = bool(getattr(args, "mvc", False))
        # rate-aware vector choice after every search (not in the reference); the encoder's choice alone
        try:
            self.mv_lambda, self.mv_iters = check_mv_refine(getattr(args, "mv_lambda", 0) or 0,
                                                            getattr(args, "mv_iters", 2) or 2)
        except ValueError as e:
            raise ValueError(f"--mv_lambda / --mv_iters: {e}") from None
        self.prefix = resolve_prefix(args.output) if getattr(args, "output", None) else None
        self.group = group if group is not None else shard.Group()

    def bye(self):
        if getattr(self, "N_frames", 0) and hasattr(self, "total_bits"):
            bpp = self.total_bits / (self.N_frames * self.width * self.height)
            logging.info(f"Output bit-rate = {bpp:.4f} bits/pixel")

    # IPP_DCT.py:595-626: encode_fn to the frame's files, decode_fn back (in memory)
    def encode_decode_proxy(self, img, frame_type, seq_idx):
        return self._code_frame(img, f"{self.prefix}_{frame_type}_{seq_idx}_enc")

    def _search(self, ref, cur, **kw):
        """The motion search of cur in ref and, with --mv_lambda, the rate-aware refinement of its field."""
        bs = self.block_size_ME
        mv = K.block_matching(ref, cur, bs, self.search_range, self.use_fast, **kw)
        if self.mv_lambda:   # at 0 the calls are what they were
            mv = K.refine_field(ref, cur, mv, bs, self.subpel, self.mv_lambda, self.mv_iters)
        return mv

    def _ws_bytes(self, H, W):
        """The searches' workspace in the resident loops: the gray planes (and the pyramids), shared
        with the refinement, whose second field overlays what the search no longer needs."""
        n = hier_workspace_bytes(H, W, self.me_levels) if self.me_levels else 2 * H * W
        return max(n, mv_refine_workspace_bytes(H, W, self.block_size_ME)) if self.mv_lambda else n

    def _gop(self, frames, g0, i_idx, p0):
        """One GOP: I-frame then P-frames (IPP.temporal_filter :397-575)."""
        if self.bframes:
            return self._gop_bframes(frames, g0, i_idx, p0)
        bs = self.block_size_ME
        recon_I, bits_I = self.encode_decode_proxy(frames[g0], "I", i_idx)
        I = {"bits": bits_I, "idx": g0}
        P, mvs, recon = [], [], [recon_I]
        ref = recon_I
        for p in range(1, min(self.gop_size, len(frames) - g0)):
            cur = frames[g0 + p]
            lv = {"levels": self.me_levels} if self.me_levels else {}   # at 0 the calls are what they were
            ob = {"obmc": True} if self.obmc else {}                    # and without --obmc
            if self.subpel > 1:
                mv = self._search(ref, cur, subpel=self.subpel, **lv)
                comp = K.motion_compensate(ref, mv, bs, subpel=self.subpel, **ob)
            else:
                mv = self._search(ref, cur, **lv)
                comp = K.motion_compensate(ref, mv, bs, **ob)
            if self.rdo_lambda > 0:
                # :441-536: per-block I/P decision, the mixed-mode frame, its reconstruction
                modes = K.rdo_modes(cur, comp, bs, self.QSS, self.rdo_lambda)
                res = K.rdo_residual(cur, comp, modes, bs)
                rec_res, bits_P = self.encode_decode_proxy(res, "P", p0 + p - 1)
                ref = K.rdo_reconstruct(comp, rec_res, modes, bs)
                n_i = int(modes.sum())
                logging.info(f"  RDO (λ={self.rdo_lambda}): {n_i}/{modes.size} I-blocks, "
                             f"{modes.size - n_i}/{modes.size} P-blocks")
                mvs.append({"mv": mv, "modes": modes})
            else:
                res = K.residual(cur, comp)
                rec_res, bits_P = self.encode_decode_proxy(res, "P", p0 + p - 1)
                ref = K.reconstruct(comp, rec_res)
                mvs.append(mv)
            P.append({"bits": bits_P})
            recon.append(ref)
        return I, P, mvs, recon

    def _b0(self, g0):
        """The first B file index of the GOP at g0: every GOP before it is full."""
        return (g0 // self.gop_size) * gop_types(self.gop_size, self.bframes).count("B")

    def _gop_bframes(self, frames, g0, i_idx, p0):
        """One GOP with B-frames: I, then per anchor interval the closing anchor (predicted from the
        anchor before it) and the B-frames between in display order (predicted from both)."""
        bs = self.block_size_ME
        kw = {"subpel": self.subpel} if self.subpel > 1 else {}
        sw = {**kw, "levels": self.me_levels} if self.me_levels else kw   # the searches' keywords
        cw = {**kw, "obmc": True} if self.obmc else kw                    # the compensations'
        types = gop_types(min(self.gop_size, len(frames) - g0), self.bframes)
        n_b = self._b0(g0)
        recon_I, bits_I = self.encode_decode_proxy(frames[g0], "I", i_idx)
        I = {"bits": bits_I, "idx": g0}
        P, mvs, recon = [], [], {0: recon_I}
        B = {"info": [], "mv": [], "modes": []}
        for a, c in _anchor_intervals(types):
            cur = frames[g0 + c]
            mv = self._search(recon[a], cur, **sw)
            comp = K.motion_compensate(recon[a], mv, bs, **cw)
            rec_res, bits_P = self.encode_decode_proxy(K.residual(cur, comp), "P", p0 + len(P))
            recon[c] = K.reconstruct(comp, rec_res)
            mvs.append(mv)
            P.append({"bits": bits_P})
            for d in range(a + 1, c):
                cur = frames[g0 + d]
                mv_f = self._search(recon[a], cur, **sw)
                mv_b = self._search(recon[c], cur, **sw)
                cf = K.motion_compensate(recon[a], mv_f, bs, **cw)
                cb = K.motion_compensate(recon[c], mv_b, bs, **cw)
                modes, res = K.bipred_residual(cur, cf, cb, bs)
                _, bits_B = self.encode_decode_proxy(res, "B", n_b)   # nothing predicts from a B-frame
                n_b += 1
                B["info"].append({"bits": bits_B})
                B["mv"].append(np.stack([mv_f, mv_b]))
                B["modes"].append(modes)
        return I, P, mvs, [recon[i] for i in sorted(recon)], B

    def encode(self):
        g = self.group
        frames = read_frames(str(self.args.input), int(self.args.number_of_frames))
        if len(frames) < 2:
            raise ValueError("Need at least 2 frames for IPP structure")
        self.N_frames = len(frames)
        self.height, self.width = frames[0].shape[:2]
        _ensure_dir(self.prefix)
        n_gops = (len(frames) + self.gop_size - 1) // self.gop_size
        lo, hi = shard.frame_range(n_gops, g.rank, g.world)
        # the originals' PNG dumps (:641-644) run beside the coding
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=4) as dumps:
            pending = [dumps.submit(write_image, f"{self.prefix}_O_{idx:04d}.png", frames[idx])
                       for idx in range(lo * self.gop_size, min(hi * self.gop_size, len(frames)))]
            local = []
            for gi in range(lo, hi):
                g0 = gi * self.gop_size
                # the P files before this GOP: every GOP before it is full
                local.append(self._gop(frames, g0, gi, gi * gop_types(self.gop_size, self.bframes).count("P")))
            for f in pending:
                f.result()
        # gather per-GOP results on rank 0 (sizes as JSON, motion fields as bytes)
        nb = self.bframes
        blob = json.dumps([[r[0], r[1]] + ([r[4]["info"]] if nb else []) for r in local]).encode()
        rdo = self.rdo_lambda > 0
        mv_of = (lambda m: m["mv"]) if rdo else (lambda m: m)
        mvbytes = b"".join(mv_of(m).astype(np.float32).tobytes() for r in local for m in r[2])
        infos = self._gather(blob)
        mvs_all = self._gather(mvbytes)
        if rdo:
            modes_all = self._gather(b"".join(m["modes"].tobytes() for r in local for m in r[2]))
        if nb:
            bmv_all = self._gather(b"".join(m.astype(np.float32).tobytes() for r in local for m in r[4]["mv"]))
            bmodes_all = self._gather(b"".join(m.astype(np.uint8).tobytes() for r in local for m in r[4]["modes"]))
        if g.rank != 0:
            return None
        I_infos, P_infos, B_infos = [], [], []
        for b in infos:
            for I, P, *rest in json.loads(b):
                I_infos.append(I)
                P_infos.extend(P)
                B_infos.extend(rest[0] if rest else [])
        hb, wb = self.height // self.block_size_ME, self.width // self.block_size_ME
        mv = np.frombuffer(b"".join(mvs_all), np.float32).reshape(len(P_infos), hb, wb, 2)
        mv_path = f"{self.prefix}_mv.vmv" if self.mvc else f"{self.prefix}_mv.npz"
        if self.mvc:
            mvfile.write(mv_path, mv, self.subpel,
                         bmv=np.frombuffer(b"".join(bmv_all), np.float32).reshape(len(B_infos), 2, hb, wb, 2) if nb else None,
                         modes=np.frombuffer(b"".join(modes_all), np.uint8).reshape(len(P_infos), hb, wb) if rdo else
                         np.frombuffer(b"".join(bmodes_all), np.uint8).reshape(len(B_infos), hb, wb) if nb else None)
        elif rdo:
            # the reference's entries are {"mv": field, "modes": map} (:529)
            modes = np.frombuffer(b"".join(modes_all), np.uint8).reshape(len(P_infos), hb, wb)
            obj = np.empty(len(P_infos), dtype=object)
            for i in range(len(P_infos)):
                obj[i] = {"mv": mv[i], "modes": modes[i]}
            np.savez_compressed(mv_path, mv=obj, mv_f32=mv, modes_u8=modes)
        else:
            obj = np.empty(len(P_infos), dtype=object)
            for i in range(len(P_infos)):
                obj[i] = mv[i]
            extra = {}
            if nb:
                extra["bmv_f32"] = np.frombuffer(b"".join(bmv_all), np.float32).reshape(len(B_infos), 2, hb, wb, 2)
                extra["bmodes_u8"] = np.frombuffer(b"".join(bmodes_all), np.uint8).reshape(len(B_infos), hb, wb)
            np.savez_compressed(mv_path, mv=np.array(list(obj), dtype=object), mv_f32=mv, **extra)
        total_bits = sum(i["bits"] for i in I_infos) + sum(p["bits"] for p in P_infos)
        total_bits += sum(b["bits"] for b in B_infos)
        total_bits += os.path.getsize(mv_path) * 8
        self.total_bits = total_bits
        meta = {"n_frames": self.N_frames, "width": self.width, "height": self.height, "gop_size": self.gop_size,
                "total_bits": total_bits, "I_info": I_infos, "P_info": P_infos,
                "mv_file": os.path.basename(mv_path), "base_prefix": os.path.basename(self.prefix)}
        if self.mvc:
            meta["mv_codec"] = mvfile.CODEC   # the coded motion file: the decoder dispatches on it
        if self.subpel > 1:
            meta["subpel"] = self.subpel   # fractional vectors: the decoder must interpolate
        if self.obmc:
            meta["obmc"] = True   # overlapped compensation: the decoder must blend alike
        if nb:
            meta["bframes"] = nb
            meta["frame_types"] = sequence_types(self.N_frames, self.gop_size, nb)
            meta["B_info"] = B_infos
        with open(f"{self.prefix}_meta.json", "w") as f:
            json.dump(meta, f, indent=4)
        return total_bits

    def _gather(self, blob: bytes):
        """Rank 0: every rank's blob in rank order (item r belongs to rank r)."""
        return self.group.gather_blobs(blob)

    def decode(self):
        in_prefix = resolve_prefix(self.args.input)
        with open(f"{in_prefix}_meta.json") as f:
            meta = json.load(f)
        mv_path = f"{os.path.dirname(in_prefix)}/{meta['mv_file']}"
        mvs, modes, bmv, bmodes = self._read_motion(mv_path, meta)
        out_prefix = resolve_prefix(self.args.output)
        _ensure_dir(out_prefix)
        gop, N = meta["gop_size"], meta["n_frames"]
        bs = self.block_size_ME
        subpel = int(meta.get("subpel", 1))
        obmc = bool(meta.get("obmc", False))
        if obmc:
            try:
                check_obmc_bs(bs)
            except ValueError:
                raise ValueError(f"meta.json: obmc with -M {bs}: -M must be 4, 8, 16, 32 or 64") from None
        ob = {"obmc": True} if obmc else {}
        if "bframes" in meta:
            recon = self._decode_bframes(meta, in_prefix, mvs, bmv, bmodes, subpel, obmc)
            return self._write_decoded(out_prefix, recon)
        recon, p_idx = [], 0
        for i_idx, g0 in enumerate(range(0, N, gop)):
            if i_idx >= len(meta["I_info"]):
                break
            ref = self._decode_frame(f"{in_prefix}_I_{i_idx}_enc")
            recon.append(ref)
            for p in range(1, min(gop, N - g0)):
                rec_res = self._decode_frame(f"{in_prefix}_P_{p_idx}_enc")
                pred = K.motion_compensate(ref, mvs[p_idx], bs, subpel=subpel, **ob) if subpel > 1 else \
                    K.motion_compensate(ref, mvs[p_idx], bs, **ob)
                if modes is not None:   # RDO was used: mode-aware reconstruction (:770-790)
                    ref = K.rdo_reconstruct(pred, rec_res, modes[p_idx], bs)
                else:
                    ref = K.reconstruct(pred, rec_res)
                recon.append(ref)
                p_idx += 1
        return self._write_decoded(out_prefix, recon)

    def _read_motion(self, mv_path, meta):
        """(P fields, -R mode maps or None, B fields or None, B mode maps or None) of the motion file,
        by meta.json's "mv_codec": absent, the .npz; "median-eg0", the coded file (mvfile.py)."""
        codec = meta.get("mv_codec")
        if codec is None:
            with np.load(mv_path, allow_pickle=False) as z:
                if "mv_f32" not in z.files:
                    raise NotImplementedError(f"{mv_path}: motion fields stored only as a pickled object array "
                                              "(written by the reference); re-encode or convert to 'mv_f32'")
                return (z["mv_f32"], z["modes_u8"] if "modes_u8" in z.files else None,
                        z["bmv_f32"] if "bmv_f32" in z.files else None,
                        z["bmodes_u8"] if "bmodes_u8" in z.files else None)
        if codec != mvfile.CODEC:
            raise NotImplementedError(f"meta.json: mv_codec {codec!r} ({mvfile.CODEC!r} or absent)")
        f = mvfile.read(mv_path)
        bs = self.block_size_ME
        n_b = len(meta.get("B_info", [])) if "bframes" in meta else 0
        mvfile.check_header(f, int(meta["height"]) // bs, int(meta["width"]) // bs, int(meta.get("subpel", 1)),
                            len(meta["P_info"]), n_b)
        if n_b:
            return f["mv_f32"], None, f["bmv_f32"], f["modes"]
        return f["mv_f32"], f["modes"], None, None

    def _decode_bframes(self, meta, in_prefix, mvs, bmv, bmodes, subpel, obmc=False):
        """The frames of a --bframes stream in display order: per GOP the I-frame, then per anchor
        interval the closing anchor and the B-frames between."""
        gop, N, nb = meta["gop_size"], meta["n_frames"], meta["bframes"]
        if not (isinstance(nb, int) and 1 <= nb <= MAX_BFRAMES and isinstance(gop, int) and gop >= 1):
            raise ValueError(f"meta.json: bframes {nb!r}, gop_size {gop!r}")
        types = meta.get("frame_types")
        if types != sequence_types(N, gop, nb):
            raise ValueError(f"meta.json: frame_types {types!r} does not follow from n_frames {N}, gop_size {gop} "
                             f"and bframes {nb}")
        n_b = types.count("B")
        if bmv is None or bmodes is None or len(bmv) != n_b or len(bmodes) != n_b:
            raise ValueError("motion file: 'bmv_f32' / 'bmodes_u8' do not hold one entry per B-frame")
        if bmodes.size and int(bmodes.max()) > 2:
            raise ValueError(f"motion file: B-frame mode {int(bmodes.max())} (0, 1 or 2)")
        bs = self.block_size_ME
        kw = {"subpel": subpel} if subpel > 1 else {}
        if obmc:
            kw["obmc"] = True
        recon, p_idx, b_idx = {}, 0, 0
        for i_idx, g0 in enumerate(range(0, N, gop)):
            if i_idx >= len(meta["I_info"]):
                break
            recon[g0] = self._decode_frame(f"{in_prefix}_I_{i_idx}_enc")
            for a, c in _anchor_intervals(types[g0:g0 + gop]):
                rec_res = self._decode_frame(f"{in_prefix}_P_{p_idx}_enc")
                recon[g0 + c] = K.reconstruct(K.motion_compensate(recon[g0 + a], mvs[p_idx], bs, **kw), rec_res)
                p_idx += 1
                for d in range(a + 1, c):
                    rec_res = self._decode_frame(f"{in_prefix}_B_{b_idx}_enc")
                    cf = K.motion_compensate(recon[g0 + a], bmv[b_idx, 0], bs, **kw)
                    cb = K.motion_compensate(recon[g0 + c], bmv[b_idx, 1], bs, **kw)
                    recon[g0 + d] = K.bipred_reconstruct(cf, cb, bmodes[b_idx], rec_res, bs)
                    b_idx += 1
        return [recon[i] for i in sorted(recon)]

    def _write_decoded(self, out_prefix, recon):
        for idx, img in enumerate(recon):
            write_image(f"{out_prefix}_{idx:04d}.png", img)
        logging.warning("decoded MP4 not written (needs PyAV/imageio, not installed); PNG frames are")
        self.recon = recon
        return len(recon)



class CoDec(_IPP, DCTCoDec):
    """IPP over 2D-DCT (the default --st).

    The GOP loop keeps every frame of the chain on the GPU (_gop_resident):
    the current frame is uploaded once, motion search, compensation,
    residual (or the -R mixed frame), transform + quantizer, the decoder's
    reconstruction and the next reference never leave HBM; only the indices
    (for the TIFF files), the motion field and the mode map come back, and
    their deflate + file writes run on a thread pool while the GPU carries on
    with the next frame.  A subclass that overrides encode_decode_proxy (or
    swaps the tools module) gets the frame-by-frame host loop of _IPP._gop."""

    def _code_frame(self, img, base):
        k = self.encode_indices(img)
        size = self._write_coded(base, k, img.shape)
        recon = self.decode_indices(k, img.shape)
        return recon, size

    def _write_coded(self, base, k, shape):
        with open(f"{base}_shape.bin", "wb") as f:
            f.write(struct.pack("iii", *shape))
        return self.encode_write_fn(self.compress(k), base)

    def _gop(self, frames, g0, i_idx, p0):
        if type(self).encode_decode_proxy is not _IPP.encode_decode_proxy or getattr(K, "__name__", "") != \
                "vcf_amd.ipp":
            return _IPP._gop(self, frames, g0, i_idx, p0)
        return self._gop_resident(frames, g0, i_idx, p0)

    def _gop_resident_bframes(self, frames, g0, i_idx, p0):
        """_gop_bframes with the chain in HBM: both anchors' reconstructions stay on the device, a
        B-frame is uploaded after its closing anchor is coded, and only the indices, the two
        fields and the mode map come back."""
        import ctypes
        from concurrent.futures import ThreadPoolExecutor
        from .. import _lib
        from .. import dct as D
        from ..device import DeviceBuffer, Stream
        H, W = frames[g0].shape[:2]
        bs, n = self.block_size_ME, H * W * 3
        Hp, Wp = D.padded_shape(H, W, self.block_size)
        hb, wb = H // bs, W // bs
        types = gop_types(min(self.gop_size, len(frames) - g0), self.bframes)
        n_b = self._b0(g0)
        s = Stream()
        cur, past, future, cf, cb, res, rec = (DeviceBuffer(n) for _ in range(7))
        nws = self._ws_bytes(H, W)
        dk, dgray = DeviceBuffer(Hp * Wp * 3), DeviceBuffer(nws)
        dmv, dmv_b, dmodes = DeviceBuffer(max(1, hb * wb * 8)), DeviceBuffer(max(1, hb * wb * 8)), \
            DeviceBuffer(max(1, hb * wb))
        q, flags, B = self.QSS, self.flags, self.block_size
        call, sh = _lib.call, s.handle
        sr, fast = int(self.search_range), int(bool(self.use_fast))

        def upload(img):
            a = np.ascontiguousarray(img, np.uint8)
            if a.shape != (H, W, 3):
                raise ValueError("IPP frames must share one H x W x 3 uint8 shape")
            call("vcf_memcpy_htod", cur.ptr, a.ctypes.data_as(ctypes.c_void_p), n, sh)
            s.synchronize()   # the host array may be freed after this

        def code(src, base, pool, decode):
            """transform + quantizer of src, indices to the host for the files; decode: decoder's frame -> rec."""
            D.encode_device(src, 1, H, W, q, flags, out=dk, stream=s, block_size=B)
            k = np.empty((Hp, Wp, 3), np.uint8)
            call("vcf_memcpy_dtoh", k.ctypes.data_as(ctypes.c_void_p), dk.ptr, k.nbytes, sh)
            if decode:
                D.decode_device(dk, 1, H, W, q, flags, out=rec, stream=s, block_size=B)
            s.synchronize()
            return pool.submit(self._write_coded, base, k, (H, W, 3))

        def predict(ref, field, comp):
            """the search of cur in ref -> field (device), the compensation -> comp, the field -> host."""
            if self.me_levels:
                call("vcf_ipp_block_match_hier", ref.ptr, cur.ptr, H, W, bs, sr, self.me_levels, self.subpel,
                     field.ptr, dgray.ptr, nws, sh)
            elif self.subpel > 1:
                call("vcf_ipp_block_match_subpel", ref.ptr, cur.ptr, H, W, bs, sr, fast, self.subpel, field.ptr,
                     dgray.ptr, sh)
            else:
                call("vcf_ipp_block_match", ref.ptr, cur.ptr, H, W, bs, sr, fast, field.ptr, dgray.ptr, sh)
            if self.mv_lambda:
                call("vcf_ipp_mv_refine", ref.ptr, cur.ptr, H, W, bs, self.subpel, self.mv_lambda, self.mv_iters,
                     field.ptr, dgray.ptr, nws, sh)
            call(mc_entry(self.subpel, self.obmc), ref.ptr, field.ptr, H, W, bs, comp.ptr, sh)
            mv = np.zeros((hb, wb, 2), np.float32)
            if mv.size:
                call("vcf_memcpy_dtoh", mv.ctypes.data_as(ctypes.c_void_p), field.ptr, mv.nbytes, sh)
            return mv

        mvs, Bs = [], {"info": [], "mv": [], "modes": []}
        try:
            with ThreadPoolExecutor(max_workers=8) as pool:
                upload(frames[g0])
                fut_I = code(cur, f"{self.prefix}_I_{i_idx}_enc", pool, True)
                call("vcf_memcpy_dtod", past.ptr, rec.ptr, n, sh)
                futs_P, futs_B = [], []
                for a, c in _anchor_intervals(types):
                    upload(frames[g0 + c])
                    mvs.append(predict(past, dmv, cf))
                    call("vcf_ipp_residual", cur.ptr, cf.ptr, n, res.ptr, sh)
                    futs_P.append(code(res, f"{self.prefix}_P_{p0 + len(futs_P)}_enc", pool, True))
                    call("vcf_ipp_reconstruct", cf.ptr, rec.ptr, n, future.ptr, sh)
                    for d in range(a + 1, c):
                        upload(frames[g0 + d])
                        mv_f, mv_b = predict(past, dmv, cf), predict(future, dmv_b, cb)
                        call("vcf_ipp_bipred_residual", cur.ptr, cf.ptr, cb.ptr, H, W, bs, dmodes.ptr, res.ptr, sh)
                        modes = np.zeros((hb, wb), np.uint8)
                        if modes.size:
                            call("vcf_memcpy_dtoh", modes.ctypes.data_as(ctypes.c_void_p), dmodes.ptr, modes.nbytes,
                                 sh)
                        futs_B.append(code(res, f"{self.prefix}_B_{n_b}_enc", pool, False))
                        n_b += 1
                        Bs["mv"].append(np.stack([mv_f, mv_b]))
                        Bs["modes"].append(modes)
                    past, future = future, past
                s.synchronize()
                I = {"bits": fut_I.result(), "idx": g0}
                P = [{"bits": f.result()} for f in futs_P]
                Bs["info"] = [{"bits": f.result()} for f in futs_B]
        finally:
            for b in (cur, past, future, cf, cb, res, rec, dk, dgray, dmv, dmv_b, dmodes):
                b.free()
            s.close()
        return I, P, mvs, [], Bs

    def _gop_resident(self, frames, g0, i_idx, p0):
        if self.bframes:
            return self._gop_resident_bframes(frames, g0, i_idx, p0)
        import ctypes
        from concurrent.futures import ThreadPoolExecutor
        from .. import _lib
        from .. import dct as D
        from ..device import DeviceBuffer, Stream
        H, W = frames[g0].shape[:2]
        bs, n = self.block_size_ME, H * W * 3
        Hp, Wp = D.padded_shape(H, W, self.block_size)
        hb, wb = H // bs, W // bs
        s = Stream()
        cur, ref, comp, res, rec = (DeviceBuffer(n) for _ in range(5))
        nws = self._ws_bytes(H, W)
        dk, dmv, dgray = DeviceBuffer(Hp * Wp * 3), DeviceBuffer(max(1, hb * wb * 8)), DeviceBuffer(nws)
        dmodes = DeviceBuffer(max(1, hb * wb))
        q, flags, B = self.QSS, self.flags, self.block_size
        call, sh = _lib.call, s.handle

        def upload(img):
            a = np.ascontiguousarray(img, np.uint8)
            if a.shape != (H, W, 3):
                raise ValueError("IPP frames must share one H x W x 3 uint8 shape")
            call("vcf_memcpy_htod", cur.ptr, a.ctypes.data_as(ctypes.c_void_p), n, sh)
            s.synchronize()   # the host array may be freed after this

        def code(src, base, pool):
            """transform + quantizer of src, indices to the host for the files, decoder's frame -> rec."""
            D.encode_device(src, 1, H, W, q, flags, out=dk, stream=s, block_size=B)
            k = np.empty((Hp, Wp, 3), np.uint8)
            call("vcf_memcpy_dtoh", k.ctypes.data_as(ctypes.c_void_p), dk.ptr, k.nbytes, sh)
            D.decode_device(dk, 1, H, W, q, flags, out=rec, stream=s, block_size=B)
            s.synchronize()
            return pool.submit(self._write_coded, base, k, (H, W, 3))

        P, mvs = [], []
        try:
            with ThreadPoolExecutor(max_workers=8) as pool:
                upload(frames[g0])
                fut_I = code(cur, f"{self.prefix}_I_{i_idx}_enc", pool)
                call("vcf_memcpy_dtod", ref.ptr, rec.ptr, n, sh)
                futs = []
                for p in range(1, min(self.gop_size, len(frames) - g0)):
                    upload(frames[g0 + p])
                    if self.me_levels:
                        call("vcf_ipp_block_match_hier", ref.ptr, cur.ptr, H, W, bs, int(self.search_range),
                             self.me_levels, self.subpel, dmv.ptr, dgray.ptr, nws, sh)
                    elif self.subpel > 1:
                        call("vcf_ipp_block_match_subpel", ref.ptr, cur.ptr, H, W, bs, int(self.search_range),
                             int(bool(self.use_fast)), self.subpel, dmv.ptr, dgray.ptr, sh)
                    else:
                        call("vcf_ipp_block_match", ref.ptr, cur.ptr, H, W, bs, int(self.search_range),
                             int(bool(self.use_fast)), dmv.ptr, dgray.ptr, sh)
                    if self.mv_lambda:
                        call("vcf_ipp_mv_refine", ref.ptr, cur.ptr, H, W, bs, self.subpel, self.mv_lambda,
                             self.mv_iters, dmv.ptr, dgray.ptr, nws, sh)
                    call(mc_entry(self.subpel, self.obmc), ref.ptr, dmv.ptr, H, W, bs, comp.ptr, sh)
                    mv = np.zeros((hb, wb, 2), np.float32)
                    if mv.size:
                        call("vcf_memcpy_dtoh", mv.ctypes.data_as(ctypes.c_void_p), dmv.ptr, mv.nbytes, sh)
                    if self.rdo_lambda > 0:
                        # :441-536: per-block I/P decision, the mixed-mode frame, its reconstruction
                        modes = np.zeros((hb, wb), np.uint8)
                        if modes.size:
                            call("vcf_ipp_rdo_modes", cur.ptr, comp.ptr, H, W, bs, int(q), float(self.rdo_lambda),
                                 dmodes.ptr, None, sh)
                            call("vcf_memcpy_dtoh", modes.ctypes.data_as(ctypes.c_void_p), dmodes.ptr, modes.nbytes,
                                 sh)
                        call("vcf_ipp_rdo_residual", cur.ptr, comp.ptr, dmodes.ptr, H, W, bs, res.ptr, sh)
                        futs.append(code(res, f"{self.prefix}_P_{p0 + p - 1}_enc", pool))
                        call("vcf_ipp_rdo_reconstruct", comp.ptr, rec.ptr, dmodes.ptr, H, W, bs, ref.ptr, sh)
                        n_i = int(modes.sum())
                        logging.info(f"  RDO (λ={self.rdo_lambda}): {n_i}/{modes.size} I-blocks, "
                                     f"{modes.size - n_i}/{modes.size} P-blocks")
                        mvs.append({"mv": mv, "modes": modes})
                    else:
                        call("vcf_ipp_residual", cur.ptr, comp.ptr, n, res.ptr, sh)
                        futs.append(code(res, f"{self.prefix}_P_{p0 + p - 1}_enc", pool))
                        call("vcf_ipp_reconstruct", comp.ptr, rec.ptr, n, ref.ptr, sh)
                        mvs.append(mv)
                s.synchronize()
                I = {"bits": fut_I.result(), "idx": g0}
                P = [{"bits": f.result()} for f in futs]
        finally:
            for b in (cur, ref, comp, res, rec, dk, dmv, dgray, dmodes):
                b.free()
            s.close()
        return I, P, mvs, []

    def _decode_frame(self, base):
        data = self.decode_read_fn(base)
        with open(f"{base}_shape.bin", "rb") as f:
            shape = struct.unpack("iii", f.read(12))
        return self.decode_indices(self.decompress(data), shape)


class CoDecDWT(_IPP, DWTCoDec):
    """IPP over 2D-DWT (--st 2D-DWT): each frame's 3l+1 subband TIFFs
    ({base}_LL_l.tif, {base}_{LH,HL,HH}_r.tif, 2D-DWT.py:162-200).  The
    reconstruction is waverec2's 2*ceil(H/2) x 2*ceil(W/2), as in the
    reference (whose IPP loop therefore needs even frame sides)."""

    def _code_frame(self, img, base):
        from .. import dwt as DW
        if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
            raise ValueError("Input image must be a 3D array (height, width, channels).")
        sb = DW.encode(img, self.wavelet, self.levels, self.QSS)[0]
        size = self.write_decom_fn(sb, base)
        H, W = self._geometry(sb)
        return DW.decode(sb, H, W, self.wavelet, self.levels, self.QSS), size

    def _decode_frame(self, base):
        from .. import dwt as DW
        sb = self.read_decom_fn(base)
        H, W = self._geometry(sb)
        return DW.decode(sb, H, W, self.wavelet, self.levels, self.QSS)


def codec_class(space_transform: str = "2D-DCT"):
    """The IPP codec class over the spatial codec --st names (IPP_DCT.py:45-87)."""
    if space_transform == "2D-DCT":
        return CoDec
    if space_transform == "2D-DWT":
        return CoDecDWT
    raise NotImplementedError(f"--st {space_transform}: 2D-DCT and 2D-DWT are on the HIP path")

"""Time the two B-frame kernels and measure what --bframes does to the coded bytes.

Kernels: one 4K B-frame (frames 0, 1, 2 of the generator of tests/subpel_ref.py; frame 1 coded from
the quarter-pel compensations of frames 0 and 2) at bs 16, resident in HBM; HIP events on the launch
stream around N launches (default 10) after a settling run past the clock ramp, median of R rounds
(default 5); in the same run, alternating, vcf_ipp_bipred_residual against vcf_ipp_residual and
vcf_ipp_bipred_reconstruct against vcf_ipp_reconstruct on the same buffers.  The floor is the
kernel's algorithmic bytes at 8 TB/s: three frames read and one written (4 frames) for the encoder
kernel, the same plus the mode bytes for the decoder kernel; the two-source kernels move 3 frames.
The decoder kernel does not read a source that a unit does not predict from, so it is timed twice:
on the encoder's own mode map, and on a map of averages only, which reads every byte the floor counts.

Bytes: 16 frames of 1080p from the same generator through IPP_DCT encode + decode (GOP 10, bs 16,
S 8, full search, --subpel 4, one -q, default 32) at --bframes 0, 1 and 2: coded bytes (the frames'
TIFFs and the motion file) and the RMSE of the decoded frames.  No threshold: the ratios against
--bframes 0 of the same run are reported, gain or loss.  Synthetic frames only.

python scripts/bench_bframes.py [N] [R] [--q Q] [--out profiles/bframes_bench.json]
"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import subpel_ref as R
from vcf_amd import _lib
from vcf_amd.codec import parser as P
from vcf_amd.codec.ipp import CoDec
from vcf_amd.device import DeviceBuffer, Event, Stream, set_device

HBM_PEAK = 8.0e12                # specified


def timed_pair(fns, s, n, rounds, settle_s=1.0):
    """The launches of fns alternating round by round -> one timing dict per fn."""
    t0 = time.time()
    while time.time() - t0 < settle_s:   # past the clock ramp
        for fn in fns:
            fn()
        s.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            e0, e1 = Event(), Event()
            e0.record(s)
            for _ in range(n):
                fn()
            e1.record(s)
            s.synchronize()
            ts[i].append(e0.elapsed_ms(e1) / n)
    return [dict(ms_per_launch=float(np.median(t)), ms_min=float(min(t)), ms_max=float(max(t))) for t in ts]


def kernel_bench(n, rounds):
    H, W, bs, sr = 2160, 3840, 16, 8
    f0, f1, f2 = R.subpel_sequence(H, W, 3, seed=1)
    s = Stream()
    sh, call = s.handle, _lib.call
    past, cur, future = (DeviceBuffer.from_array(a) for a in (f0, f1, f2))
    cf, cb, res, out = (DeviceBuffer(f0.nbytes) for _ in range(4))
    hb, wb = H // bs, W // bs
    mv, gray, modes = DeviceBuffer(hb * wb * 8), DeviceBuffer(2 * H * W), DeviceBuffer(hb * wb)
    for ref, comp in ((past, cf), (future, cb)):
        call("vcf_ipp_block_match_subpel", ref.ptr, cur.ptr, H, W, bs, sr, 0, 4, mv.ptr, gray.ptr, sh)
        call("vcf_ipp_motion_compensate_qpel", ref.ptr, mv.ptr, H, W, bs, comp.ptr, sh)
    nb = f0.nbytes
    avg = DeviceBuffer.from_array(np.full(hb * wb, 2, np.uint8))
    out_res = dict(H=H, W=W, bs=bs, sr=sr, subpel=4, launches=n, rounds=rounds, frame_bytes=nb, mode_bytes=hb * wb,
                   note="the timed buffers (about 100 MB) stay resident in the 256 MiB Infinity Cache between launches: "
                        "fraction_of_floor compares with the algorithmic bytes at the 8 TB/s HBM rate, it is not a "
                        "measured share of HBM bandwidth")
    pairs = {
        "encoder": (("bipred_residual", 4 * nb,
                     lambda: call("vcf_ipp_bipred_residual", cur.ptr, cf.ptr, cb.ptr, H, W, bs, modes.ptr, res.ptr, sh)),
                    ("residual", 3 * nb, lambda: call("vcf_ipp_residual", cur.ptr, cf.ptr, nb, res.ptr, sh))),
        "decoder": (("bipred_reconstruct", 4 * nb + hb * wb,
                     lambda: call("vcf_ipp_bipred_reconstruct", cf.ptr, cb.ptr, modes.ptr, res.ptr, H, W, bs, out.ptr,
                                  sh)),
                    ("reconstruct", 3 * nb, lambda: call("vcf_ipp_reconstruct", cf.ptr, res.ptr, nb, out.ptr, sh)),
                    ("bipred_reconstruct_all_average", 4 * nb + hb * wb,
                     lambda: call("vcf_ipp_bipred_reconstruct", cf.ptr, cb.ptr, avg.ptr, res.ptr, H, W, bs, out.ptr,
                                  sh))),
    }
    for side in ("encoder", "decoder"):   # the encoder first: the decoder kernels read its modes and residual
        ts = timed_pair([fn for _, _, fn in pairs[side]], s, n, rounds)
        base = ts[1]                      # the two-source kernel of the pair
        for (name, nbytes, _), t in zip(pairs[side], ts):
            floor_ms = nbytes / HBM_PEAK * 1e3
            t.update(algorithmic_bytes=nbytes, floor_ms_at_8tb=floor_ms, fraction_of_floor=floor_ms / t["ms_per_launch"],
                     gb_per_s=nbytes / (t["ms_per_launch"] * 1e-3) / 1e9)
            if t is not base:
                t[f"over_{pairs[side][1][0]}"] = t["ms_per_launch"] / base["ms_per_launch"]
            out_res[name] = t
    m = modes.download(np.empty((hb, wb), np.uint8), s)
    s.synchronize()
    out_res["mode_share"] = [float(x) for x in np.bincount(m.reshape(-1), minlength=3) / m.size]
    for buf in (past, cur, future, cf, cb, res, out, mv, gray, modes, avg):
        buf.free()
    s.close()
    return out_res


def bytes_bench(q):
    n, H, W = 16, 1080, 1920
    frames = np.stack(R.subpel_sequence(H, W, n, seed=2))
    res = dict(frames=n, H=H, W=W, gop=10, bs=16, sr=8, q=q, subpel=4,
               source="tests/subpel_ref.py subpel_sequence, seed 2 (synthetic; no natural images measured)")
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "frames.npy"), frames)
        for N in (0, 1, 2):
            enc, dec = os.path.join(d, f"e{N}", "v"), os.path.join(d, f"d{N}", "v")
            c = CoDec(P.parse(P.ipp_parser(), ["encode", "-i", os.path.join(d, "frames.npy"), "-O", enc, "-N", str(n),
                                               "-q", str(q), "--subpel", "4", "--bframes", str(N)]))
            bits = c.encode()
            dc = CoDec(P.parse(P.ipp_parser(), ["decode", "-i", enc, "-O", dec, "-q", str(q)]))
            dc.decode()
            err = np.stack(dc.recon).astype(np.float64) - frames
            meta = json.load(open(enc + "_meta.json"))
            types = meta.get("frame_types", "".join("I" + "P" * (min(10, n - g) - 1) for g in range(0, n, 10)))
            per = np.sqrt((err ** 2).mean(axis=(1, 2, 3)))
            r = dict(coded_bytes=bits // 8, mv_file_bytes=os.path.getsize(enc + "_mv.npz"), frame_types=types,
                     p_frame_bytes=sum(p["bits"] for p in meta["P_info"]) // 8,
                     b_frame_bytes=sum(b["bits"] for b in meta.get("B_info", [])) // 8,
                     rmse=float(np.sqrt((err ** 2).mean())),
                     rmse_by_type={t: float(np.sqrt((per[[i for i, c in enumerate(types) if c == t]] ** 2).mean()))
                                   for t in sorted(set(types))})
            if N:
                with np.load(enc + "_mv.npz", allow_pickle=False) as z:
                    m = z["bmodes_u8"]
                    r["mode_share"] = [float(x) for x in np.bincount(m.reshape(-1), minlength=3) / max(1, m.size)]
            res[f"bframes_{N}"] = r
    for N in (1, 2):
        res[f"bframes_{N}"]["bytes_over_bframes_0"] = res[f"bframes_{N}"]["coded_bytes"] / res["bframes_0"]["coded_bytes"]
        res[f"bframes_{N}"]["rmse_over_bframes_0"] = res[f"bframes_{N}"]["rmse"] / res["bframes_0"]["rmse"]
    return res


def main():
    argv = sys.argv[1:]
    out, q = os.path.join(ROOT, "profiles", "bframes_bench.json"), 32
    for flag in ("--out", "--q"):
        if flag in argv:
            i = argv.index(flag)
            if flag == "--out":
                out = argv[i + 1]
            else:
                q = int(argv[i + 1])
            del argv[i:i + 2]
    n = int(argv[0]) if argv else 10
    rounds = int(argv[1]) if len(argv) > 1 else 5
    set_device(0)
    res = dict(kernel=kernel_bench(n, rounds), coding=bytes_bench(q))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

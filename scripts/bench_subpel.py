"""Time the sub-pel search and compensator and measure what --subpel does to the coded bytes.

Kernels: one 4K frame pair (the generator of tests/subpel_ref.py: true quarter-pel motion) at
bs 16, S 8, full search, resident in HBM; HIP events on the launch stream around N launches
(default 10) after a settling run past the clock ramp, median of R rounds (default 5); in the
same run vcf_ipp_block_match against vcf_ipp_block_match_subpel (N = 2, 4), and
vcf_ipp_motion_compensate against vcf_ipp_motion_compensate_qpel on the refined field (GB/s of
the frame read once and written once, and its share of 8 TB/s).

Bytes: 16 frames of 1080p from the same generator through IPP_DCT encode + decode (GOP 10, bs 16,
S 8, full search, one -q, default 32) at --subpel 1, 2 and 4: coded bytes (the frames' TIFFs and
the motion file) and the RMSE of the decoded frames.  No threshold: the ratios are reported.

python scripts/bench_subpel.py [N] [R] [--q Q] [--out profiles/subpel_bench.json]
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


def timed(fn, s, n, rounds, settle_s=1.0):
    t0 = time.time()
    while time.time() - t0 < settle_s:   # past the clock ramp
        for _ in range(2):
            fn()
        s.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = Event(), Event()
        e0.record(s)
        for _ in range(n):
            fn()
        e1.record(s)
        s.synchronize()
        ts.append(e0.elapsed_ms(e1) / n)
    return dict(ms_per_launch=float(np.median(ts)), ms_min=float(min(ts)), ms_max=float(max(ts)))


def kernel_bench(n, rounds):
    H, W, bs, sr = 2160, 3840, 16, 8
    a, b = R.subpel_sequence(H, W, 2, seed=1)
    s = Stream()
    sh, call = s.handle, _lib.call
    ref, cur, out = DeviceBuffer.from_array(a), DeviceBuffer.from_array(b), DeviceBuffer(a.nbytes)
    mv, gray = DeviceBuffer((H // bs) * (W // bs) * 8), DeviceBuffer(2 * H * W)
    res = dict(H=H, W=W, bs=bs, sr=sr, search="full", launches=n, rounds=rounds, frame_bytes=a.nbytes)
    res["block_match"] = timed(lambda: call("vcf_ipp_block_match", ref.ptr, cur.ptr, H, W, bs, sr, 0, mv.ptr,
                                            gray.ptr, sh), s, n, rounds)
    for N in (2, 4):
        t = timed(lambda: call("vcf_ipp_block_match_subpel", ref.ptr, cur.ptr, H, W, bs, sr, 0, N, mv.ptr, gray.ptr,
                               sh), s, n, rounds)
        t["over_block_match"] = t["ms_per_launch"] / res["block_match"]["ms_per_launch"]
        t["refinement_ms"] = t["ms_per_launch"] - res["block_match"]["ms_per_launch"]
        res[f"block_match_subpel_{N}"] = t
        field = mv.download(np.empty((H // bs, W // bs, 2), np.float32), s)
        s.synchronize()
        t["fractional_blocks"] = float((field != np.rint(field)).any(axis=2).mean())
        for name in ("vcf_ipp_motion_compensate", "vcf_ipp_motion_compensate_qpel"):
            if name.endswith("qpel") or N == 2:   # the whole-pel kernel truncates the field: time it once
                m = timed(lambda: call(name, ref.ptr, mv.ptr, H, W, bs, out.ptr, sh), s, n, rounds)
                rate = 2 * a.nbytes / (m["ms_per_launch"] * 1e-3)
                m.update(gb_per_s=rate / 1e9, share_of_8tb=rate / HBM_PEAK)
                res["motion_compensate" if not name.endswith("qpel") else f"motion_compensate_qpel_{N}"] = m
    for N in (2, 4):
        res[f"motion_compensate_qpel_{N}"]["over_motion_compensate"] = \
            res[f"motion_compensate_qpel_{N}"]["ms_per_launch"] / res["motion_compensate"]["ms_per_launch"]
    for buf in (ref, cur, out, mv, gray):
        buf.free()
    s.close()
    return res


def bytes_bench(q):
    n, H, W = 16, 1080, 1920
    frames = np.stack(R.subpel_sequence(H, W, n, seed=2))
    res = dict(frames=n, H=H, W=W, gop=10, bs=16, sr=8, q=q, source="tests/subpel_ref.py subpel_sequence, seed 2")
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "frames.npy"), frames)
        for N in (1, 2, 4):
            enc, dec = os.path.join(d, f"e{N}", "v"), os.path.join(d, f"d{N}", "v")
            c = CoDec(P.parse(P.ipp_parser(), ["encode", "-i", os.path.join(d, "frames.npy"), "-O", enc, "-N", str(n),
                                               "-q", str(q), "--subpel", str(N)]))
            bits = c.encode()
            dc = CoDec(P.parse(P.ipp_parser(), ["decode", "-i", enc, "-O", dec, "-q", str(q)]))
            dc.decode()
            err = np.stack(dc.recon).astype(np.float64) - frames
            meta = json.load(open(enc + "_meta.json"))
            res[f"subpel_{N}"] = dict(coded_bytes=bits // 8, mv_file_bytes=os.path.getsize(enc + "_mv.npz"),
                                      p_frame_bytes=sum(p["bits"] for p in meta["P_info"]) // 8,
                                      rmse=float(np.sqrt((err ** 2).mean())))
    for N in (2, 4):
        res[f"subpel_{N}"]["bytes_over_whole_pel"] = res[f"subpel_{N}"]["coded_bytes"] / res["subpel_1"]["coded_bytes"]
    return res


def main():
    argv = sys.argv[1:]
    out, q = os.path.join(ROOT, "profiles", "subpel_bench.json"), 32
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

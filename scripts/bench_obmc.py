"""Time the overlapped compensator and measure what --obmc does to the coded bytes and the error.

Kernel: one 4K frame pair (the generator of tests/subpel_ref.py: true quarter-pel motion), resident
in HBM, at bs 8, 16 and 32 with the quarter-pel field of vcf_ipp_block_match_subpel (S 8, full
search); vcf_ipp_motion_compensate_obmc against vcf_ipp_motion_compensate_qpel on the same buffers
in the same run, alternating: HIP events on the launch stream around N launches (default 10) after
a settling run past the clock ramp, median of R rounds (default 5).  Reported: ms per launch, the
ratio, GB/s of the frame read once and written once, and its share of 8 TB/s.  At each bs the
overlapped output under a uniform valid field is compared with the quarter-pel kernel's (it must
be equal), and the share of bytes the searched field changes is reported.

Coding: 16 frames of 1080p through IPP_DCT encode + decode (GOP 10, bs 16, S 8, -q 32) with and
without --obmc, at --subpel 1, --subpel 4 and --subpel 4 --bframes 1, for the slow sequence of
scripts/bench_subpel.py and the fast one of scripts/bench_hier.py (the latter with --me_levels 2,
without which S 8 does not reach its motion): coded bytes (the frames' TIFFs and the motion file)
and the RMSE of the decoded frames.  No threshold: the ratios are reported as they come out.

python scripts/bench_obmc.py [N] [R] [--no-coding] [--out profiles/obmc_bench.json]
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

import hier_ref
import subpel_ref as R
from vcf_amd import _lib
from vcf_amd.codec import parser as P
from vcf_amd.codec.ipp import CoDec
from vcf_amd.device import DeviceBuffer, Event, Stream, set_device

HBM_PEAK = 8.0e12                # specified
QPEL, OBMC = "vcf_ipp_motion_compensate_qpel", "vcf_ipp_motion_compensate_obmc"


def timed_pair(fns, s, n, rounds, settle_s=1.0):
    """Per-launch times of the functions of fns, taken in turn within every round."""
    t0 = time.time()
    while time.time() - t0 < settle_s:   # past the clock ramp
        for fn in fns.values():
            fn()
        s.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = Event(), Event()
            e0.record(s)
            for _ in range(n):
                fn()
            e1.record(s)
            s.synchronize()
            ts[k].append(e0.elapsed_ms(e1) / n)
    return {k: dict(ms_per_launch=float(np.median(v)), ms_min=float(min(v)), ms_max=float(max(v))) for k, v in ts.items()}


def kernel_bench(n, rounds):
    H, W, sr = 2160, 3840, 8
    a, b = R.subpel_sequence(H, W, 2, seed=1)
    s = Stream()
    sh, call = s.handle, _lib.call
    ref, cur = DeviceBuffer.from_array(a), DeviceBuffer.from_array(b)
    out = {QPEL: DeviceBuffer(a.nbytes), OBMC: DeviceBuffer(a.nbytes)}
    gray = DeviceBuffer(2 * H * W)
    res = dict(H=H, W=W, sr=sr, search="full, quarter pel", launches=n, rounds=rounds, frame_bytes=a.nbytes,
               source="tests/subpel_ref.py subpel_sequence, seed 1")

    def frames(mv, bs):
        got = {}
        for name in (QPEL, OBMC):
            call(name, ref.ptr, mv.ptr, H, W, bs, out[name].ptr, sh)
            got[name] = out[name].download(np.empty_like(a), s)
            s.synchronize()
        return got

    for bs in (8, 16, 32):
        shape = (H // bs, W // bs, 2)
        mv = DeviceBuffer(shape[0] * shape[1] * 8)
        # equal outputs under a uniform valid field (0.75, 1.25) on a frame with 2 .. bs + 1 rows and columns
        # beyond its full blocks, so that every block's vector is valid
        Hc, Wc = H - bs + 2, W - bs + 2
        uni = DeviceBuffer.from_array(np.tile(np.float32((0.75, 1.25)), (Hc // bs, Wc // bs, 1)))
        got = {}
        for name in (QPEL, OBMC):
            call(name, ref.ptr, uni.ptr, Hc, Wc, bs, out[name].ptr, sh)
            got[name] = out[name].download(np.empty(Hc * Wc * 3, np.uint8), s)
            s.synchronize()
        uniform_equal = bool(np.array_equal(got[QPEL], got[OBMC]))
        uni.free()
        call("vcf_ipp_block_match_subpel", ref.ptr, cur.ptr, H, W, bs, sr, 0, 4, mv.ptr, gray.ptr, sh)
        field = mv.download(np.empty(shape, np.float32), s)
        s.synchronize()
        got = frames(mv, bs)
        t = timed_pair({name: (lambda name=name: call(name, ref.ptr, mv.ptr, H, W, bs, out[name].ptr, sh))
                        for name in (QPEL, OBMC)}, s, n, rounds)
        for m in t.values():
            rate = 2 * a.nbytes / (m["ms_per_launch"] * 1e-3)
            m.update(gb_per_s=rate / 1e9, share_of_8tb=rate / HBM_PEAK)
        err = {k: float(((v.astype(np.float64) - b) ** 2).sum()) for k, v in got.items()}
        res[f"bs{bs}"] = dict(qpel=t[QPEL], obmc=t[OBMC], obmc_over_qpel=t[OBMC]["ms_per_launch"] / t[QPEL]["ms_per_launch"],
                              uniform_field_equals_qpel=uniform_equal,
                              fractional_blocks=float((field != np.rint(field)).any(axis=2).mean()),
                              bytes_changed=float((got[QPEL] != got[OBMC]).mean()),
                              prediction_sse_qpel=err[QPEL], prediction_sse_obmc=err[OBMC],
                              prediction_sse_ratio=err[OBMC] / err[QPEL])
        mv.free()
        print(json.dumps({f"bs{bs}": res[f"bs{bs}"]}), flush=True)
    for buf in (ref, cur, gray, *out.values()):
        buf.free()
    s.close()
    return res


CODING = {"subpel1": ["--subpel", "1"], "subpel4": ["--subpel", "4"], "subpel4_bframes1": ["--subpel", "4", "--bframes", "1"]}


def coding_bench(frames, source, extra):
    n, H, W = frames.shape[:3]
    res = dict(frames=n, H=H, W=W, gop=10, bs=16, sr=8, q=32, flags=extra, source=source)
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "frames.npy"), frames)
        for key, flags in CODING.items():
            for ob in (False, True):
                tag = key + ("_obmc" if ob else "")
                enc, dec = os.path.join(d, "e" + tag, "v"), os.path.join(d, "d" + tag, "v")
                args = ["-q", "32"] + flags + extra + (["--obmc"] if ob else [])
                bits = CoDec(P.parse(P.ipp_parser(), ["encode", "-i", os.path.join(d, "frames.npy"), "-O", enc, "-N",
                                                       str(n)] + args)).encode()
                dc = CoDec(P.parse(P.ipp_parser(), ["decode", "-i", enc, "-O", dec, "-q", "32"]))
                dc.decode()
                err = np.stack(dc.recon).astype(np.float64) - frames
                res[tag] = dict(coded_bytes=bits // 8, mv_file_bytes=os.path.getsize(enc + "_mv.npz"),
                                rmse=float(np.sqrt((err ** 2).mean())))
                print(json.dumps({tag: res[tag]}), flush=True)
            a, b = res[key + "_obmc"], res[key]
            a["bytes_over_plain"], a["rmse_over_plain"] = a["coded_bytes"] / b["coded_bytes"], a["rmse"] / b["rmse"]
    return res


def main():
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "obmc_bench.json")
    coding = "--no-coding" not in argv
    argv = [x for x in argv if x != "--no-coding"]
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    n = int(argv[0]) if argv else 10
    rounds = int(argv[1]) if len(argv) > 1 else 5
    set_device(0)
    res = dict(kernel=kernel_bench(n, rounds))
    if coding:
        n, H, W = 16, 1080, 1920
        res["coding_slow"] = coding_bench(np.stack(R.subpel_sequence(H, W, n, seed=2)),
                                          "tests/subpel_ref.py subpel_sequence, (1.25, 1.75) per frame, seed 2", [])
        res["coding_fast"] = coding_bench(np.stack(hier_ref.fast_sequence(n, H, W, (11.25, -6.75), seed=2)),
                                          "tests/hier_ref.py fast_sequence, shift (11.25, -6.75) per frame, seed 2",
                                          ["--me_levels", "2"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

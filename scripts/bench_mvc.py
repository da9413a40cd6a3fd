"""Time the rate-aware refinement of a motion field and measure what --mvc and --mv_lambda do to the
coded bytes and the error.

Kernel: one 4K frame pair (the generator of tests/subpel_ref.py: true quarter-pel motion), resident
in HBM, at bs 16 and 8, subpel 4, S 8: vcf_ipp_mv_refine (lambda 16, 2 iterations; the gray pass,
two launches) on the field of vcf_ipp_block_match_subpel, against that search on the same buffers
in the same run, alternating: HIP events on the launch stream around N launches (default 10) after
a settling run past the clock ramp, median of R rounds (default 5).  The refinement runs on a copy
of the searched field, restored before every timed launch by a device copy that is timed with it
(8 bytes per block).  Reported: ms per launch, the ratio, and the share of 8 TB/s of the bytes the
call must move at least (both RGB frames read, both gray planes written and read, the field read
and written per iteration).

Coding: 16 frames of 1080p through IPP_DCT encode + decode (GOP 10, bs 16, S 8, -q 32) under
--subpel 4, --subpel 4 --obmc and --subpel 4 --me_levels 2, for the slow high-frequency sequence
of tests/subpel_ref.py, the fast one of tests/hier_ref.py (always with --me_levels 2, without which
S 8 does not reach its motion) and the latter's texture moving slowly: the parent format (no new
flag), then --mvc with --mv_lambda 0, 4, 16 and 64: coded bytes (the frames' files and the motion
file), the motion file's bytes, and the RMSE of the decoded frames.  No threshold: the ratios are
reported as they come out.

python scripts/bench_mvc.py [N] [R] [--no-coding] [--out profiles/mvc_bench.json]
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
from vcf_amd import ipp as K
from vcf_amd.codec import parser as P
from vcf_amd.codec.ipp import CoDec
from vcf_amd.device import DeviceBuffer, Event, Stream, set_device

HBM_PEAK = 8.0e12                # specified
SEARCH, REFINE = "vcf_ipp_block_match_subpel", "vcf_ipp_mv_refine"


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
    H, W, sr, subpel, lam, it = 2160, 3840, 8, 4, 16, 2
    a, b = R.subpel_sequence(H, W, 2, seed=1)
    s = Stream()
    sh, call = s.handle, _lib.call
    ref, cur = DeviceBuffer.from_array(a), DeviceBuffer.from_array(b)
    res = dict(H=H, W=W, sr=sr, subpel=subpel, lam=lam, iterations=it, launches=n, rounds=rounds,
               source="tests/subpel_ref.py subpel_sequence, seed 1")
    for bs in (16, 8):
        shape = (H // bs, W // bs, 2)
        nb = shape[0] * shape[1]
        nws = K.mv_refine_workspace_bytes(H, W, bs)
        mv, keep, ws = DeviceBuffer(nb * 8), DeviceBuffer(nb * 8), DeviceBuffer(nws)
        call(SEARCH, ref.ptr, cur.ptr, H, W, bs, sr, 0, subpel, keep.ptr, ws.ptr, sh)
        before = keep.download(np.empty(shape, np.float32), s)
        s.synchronize()

        def refine():
            call("vcf_memcpy_dtod", mv.ptr, keep.ptr, nb * 8, sh)
            call(REFINE, ref.ptr, cur.ptr, H, W, bs, subpel, lam, it, mv.ptr, ws.ptr, nws, sh)

        refine()
        after = mv.download(np.empty(shape, np.float32), s)
        s.synchronize()
        t = timed_pair({SEARCH: lambda: call(SEARCH, ref.ptr, cur.ptr, H, W, bs, sr, 0, subpel, mv.ptr, ws.ptr, sh),
                        REFINE: refine}, s, n, rounds)
        least = 6 * H * W + 4 * H * W + it * 2 * 8 * nb
        m = t[REFINE]
        m.update(least_bytes=least, gb_per_s=least / (m["ms_per_launch"] * 1e-3) / 1e9,
                 share_of_8tb=least / (m["ms_per_launch"] * 1e-3) / HBM_PEAK)
        res[f"bs{bs}"] = dict(search=t[SEARCH], refine=m, refine_over_search=m["ms_per_launch"] / t[SEARCH]["ms_per_launch"],
                              blocks=nb, blocks_changed=float((before != after).any(axis=2).mean()))
        for buf in (mv, keep, ws):
            buf.free()
        print(json.dumps({f"bs{bs}": res[f"bs{bs}"]}), flush=True)
    for buf in (ref, cur):
        buf.free()
    s.close()
    return res


FLAGS = {"subpel4": ["--subpel", "4"], "subpel4_obmc": ["--subpel", "4", "--obmc"],
         "subpel4_me_levels2": ["--subpel", "4", "--me_levels", "2"]}
LAMBDAS = (0, 4, 16, 64)


def coding_bench(frames, source, always=()):
    n, H, W = frames.shape[:3]
    res = dict(frames=n, H=H, W=W, gop=10, bs=16, sr=8, q=32, source=source, always=list(always))
    done = {}
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "frames.npy"), frames)
        for key, flags in FLAGS.items():
            flags = flags + [f for f in always if f not in flags]
            if tuple(flags) in done:                  # the same flags under another name
                res[key] = dict(same_as=done[tuple(flags)])
                continue
            done[tuple(flags)] = key
            row = {}
            for tag, new in [("parent_format", [])] + [(f"mvc_lambda{l}", ["--mvc", "--mv_lambda", str(l)]) for l in LAMBDAS]:
                enc, dec = os.path.join(d, key + tag, "v"), os.path.join(d, "d" + key + tag, "v")
                bits = CoDec(P.parse(P.ipp_parser(), ["encode", "-i", os.path.join(d, "frames.npy"), "-O", enc, "-N", str(n),
                                                      "-q", "32"] + flags + new)).encode()
                dc = CoDec(P.parse(P.ipp_parser(), ["decode", "-i", enc, "-O", dec, "-q", "32"]))
                dc.decode()
                err = np.stack(dc.recon).astype(np.float64) - frames
                mv_file = enc + ("_mv.vmv" if new else "_mv.npz")
                row[tag] = dict(coded_bytes=bits // 8, mv_file_bytes=os.path.getsize(mv_file),
                                rmse=float(np.sqrt((err ** 2).mean())))
                base = row["parent_format"]
                row[tag].update(bytes_over_parent=row[tag]["coded_bytes"] / base["coded_bytes"],
                                mv_bytes_over_parent=row[tag]["mv_file_bytes"] / base["mv_file_bytes"],
                                rmse_over_parent=row[tag]["rmse"] / base["rmse"])
                print(json.dumps({key: {tag: row[tag]}}), flush=True)
            res[key] = row
    return res


def main():
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "mvc_bench.json")
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
        res["coding_slow_hf"] = coding_bench(np.stack(R.subpel_sequence(H, W, n, seed=2)),
                                             "tests/subpel_ref.py subpel_sequence, (1.25, 1.75) per frame, seed 2")
        res["coding_fast"] = coding_bench(np.stack(hier_ref.fast_sequence(n, H, W, (11.25, -6.75), seed=2)),
                                          "tests/hier_ref.py fast_sequence, shift (11.25, -6.75) per frame, seed 2",
                                          always=("--me_levels", "2"))
        res["coding_slow_lf"] = coding_bench(np.stack(hier_ref.fast_sequence(n, H, W, (1.25, 1.75), seed=2)),
                                             "tests/hier_ref.py fast_sequence, shift (1.25, 1.75) per frame, seed 2")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

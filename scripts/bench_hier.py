"""Time the hierarchical motion search against the plain one and measure what --me_levels does to
the coded bytes.

Search: one 4K frame pair of tests/hier_ref.py's fast_sequence (shift (19, -13)) at bs 16, resident
in HBM; HIP events on the launch stream around N launches (default 10) after a settling second,
median of R rounds (default 5), the variants alternating round by round in the same run: plain
S = 8, plain S = 32, L = 2 S = 8, L = 3 S = 8 and L = 2 S = 2, each at subpel 1 and 4.  The
hierarchical time is split by differences of whole calls, each ending in a wait on the stream
(the stages have no entry of their own): gray = the plain call at S = 0 (both gray passes and a
one-candidate search), pyramid + refinement = the hierarchical call at S = 0 minus that, top
level = the hierarchical call at S = 8 minus the one at S = 0.  The one condition: L = 2, S = 8
takes less time than plain S = 32.

Coding: 16 frames of 1080p from the same generator (shift (11.25, -6.75) per frame), and the slow
quarter-pel sequence of scripts/bench_subpel.py (tests/subpel_ref.py, seed 2), through IPP_DCT
encode + decode (GOP 10, bs 16, S 8, --subpel 4, -q 32, -c TIFF) at --bframes 0, 1, 2 x --me_levels 0, 2: coded bytes (the frames'
files and the motion file) and the RMSE of the decoded frames.  Synthetic frames only.

python scripts/bench_hier.py [N] [R] [--out profiles/hier_bench.json] [--no-coding]
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

import hier_ref as R
from vcf_amd import _lib
from vcf_amd import ipp as K
from vcf_amd.codec import parser as P
from vcf_amd.codec.ipp import CoDec
from vcf_amd.device import DeviceBuffer, Event, Stream, set_device


def search_bench(n, rounds):
    H, W, bs = 2160, 3840, 16
    a, b = R.fast_sequence(2, H, W, (19, -13), seed=1)
    s = Stream()
    sh, call = s.handle, _lib.call
    ref, cur = DeviceBuffer.from_array(a), DeviceBuffer.from_array(b)
    nws = K.hier_workspace_bytes(H, W, 3)
    mv, ws = DeviceBuffer((H // bs) * (W // bs) * 8), DeviceBuffer(nws)

    def plain(sr, subpel):
        if subpel == 1:
            return lambda: call("vcf_ipp_block_match", ref.ptr, cur.ptr, H, W, bs, sr, 0, mv.ptr, ws.ptr, sh)
        return lambda: call("vcf_ipp_block_match_subpel", ref.ptr, cur.ptr, H, W, bs, sr, 0, subpel, mv.ptr, ws.ptr, sh)

    def hier(lv, sr, subpel):
        return lambda: call("vcf_ipp_block_match_hier", ref.ptr, cur.ptr, H, W, bs, sr, lv, subpel, mv.ptr, ws.ptr,
                            nws, sh)

    variants = {}
    for sp in (1, 4):
        variants[f"plain_S8_subpel{sp}"] = plain(8, sp)
        variants[f"plain_S32_subpel{sp}"] = plain(32, sp)
        variants[f"L2_S8_subpel{sp}"] = hier(2, 8, sp)
        variants[f"L3_S8_subpel{sp}"] = hier(3, 8, sp)
        variants[f"L2_S2_subpel{sp}"] = hier(2, 2, sp)
    # the split (see the module docstring)
    variants["split_plain_S0"] = plain(0, 1)
    for lv in (2, 3):
        variants[f"split_L{lv}_S0"] = hier(lv, 0, 1)
    t0 = time.time()
    while time.time() - t0 < 1.0:            # a settling second, every variant warmed
        for fn in variants.values():
            fn()
        s.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(rounds):                  # the variants alternate round by round
        for k, fn in variants.items():
            e0, e1 = Event(), Event()
            e0.record(s)
            for _ in range(n):
                fn()
            e1.record(s)
            s.synchronize()
            ts[k].append(e0.elapsed_ms(e1) / n)
    res = dict(H=H, W=W, bs=bs, launches=n, rounds=rounds, source="tests/hier_ref.py fast_sequence, shift (19, -13), seed 1")
    res["ms"] = {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ts.items()}
    m = {k: v["median"] for k, v in res["ms"].items()}
    res["split_ms"] = {f"L{lv}_S8": dict(gray=m["split_plain_S0"], pyramid_and_refinement=m[f"split_L{lv}_S0"] - m["split_plain_S0"],
                                         top_level=m[f"L{lv}_S8_subpel1"] - m[f"split_L{lv}_S0"]) for lv in (2, 3)}
    res["L2_S8_over_plain_S8"] = {sp: m[f"L2_S8_subpel{sp}"] / m[f"plain_S8_subpel{sp}"] for sp in (1, 4)}
    res["L2_S8_over_plain_S32"] = {sp: m[f"L2_S8_subpel{sp}"] / m[f"plain_S32_subpel{sp}"] for sp in (1, 4)}
    res["condition_L2_S8_faster_than_plain_S32"] = all(v < 1.0 for v in res["L2_S8_over_plain_S32"].values())
    # what the fields find: exact (19, -13) among the blocks whose true match lies in the frame
    inside = np.array([[R.inside(by * bs - 13, bx * bs + 19, bs, H, W) for bx in range(W // bs)] for by in range(H // bs)])
    res["exact_share"] = {}
    for k in ("plain_S8_subpel1", "plain_S32_subpel1", "L2_S8_subpel1", "L3_S8_subpel1", "L2_S2_subpel1"):
        variants[k]()
        f = mv.download(np.empty((H // bs, W // bs, 2), np.float32), s)
        s.synchronize()
        res["exact_share"][k] = float((f == (19, -13)).all(axis=2)[inside].mean())
    for buf in (ref, cur, mv, ws):
        buf.free()
    s.close()
    return res


def coding_bench(frames, source):
    n, H, W = frames.shape[:3]
    res = dict(frames=n, H=H, W=W, gop=10, bs=16, sr=8, subpel=4, q=32, source=source)
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "frames.npy"), frames)
        for nb in (0, 1, 2):
            for lv in (0, 2):
                enc, dec = os.path.join(d, f"e{nb}{lv}", "v"), os.path.join(d, f"d{nb}{lv}", "v")
                flags = ["-q", "32", "--subpel", "4", "--bframes", str(nb), "--me_levels", str(lv)]
                bits = CoDec(P.parse(P.ipp_parser(), ["encode", "-i", os.path.join(d, "frames.npy"), "-O", enc, "-N",
                                                       str(n)] + flags)).encode()
                dc = CoDec(P.parse(P.ipp_parser(), ["decode", "-i", enc, "-O", dec, "-q", "32"]))
                dc.decode()
                err = np.stack(dc.recon).astype(np.float64) - frames
                res[f"bframes{nb}_levels{lv}"] = dict(coded_bytes=bits // 8, mv_file_bytes=os.path.getsize(enc + "_mv.npz"),
                                                      rmse=float(np.sqrt((err ** 2).mean())))
    for nb in (0, 1, 2):
        a, b = res[f"bframes{nb}_levels2"], res[f"bframes{nb}_levels0"]
        a["bytes_over_levels0"], a["rmse_over_levels0"] = a["coded_bytes"] / b["coded_bytes"], a["rmse"] / b["rmse"]
    return res


def main():
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "hier_bench.json")
    coding = "--no-coding" not in argv
    argv = [x for x in argv if x != "--no-coding"]
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    n = int(argv[0]) if argv else 10
    rounds = int(argv[1]) if len(argv) > 1 else 5
    set_device(0)
    res = dict(search=search_bench(n, rounds))
    if coding:
        import subpel_ref
        n, H, W = 16, 1080, 1920
        res["coding_fast"] = coding_bench(np.stack(R.fast_sequence(n, H, W, (11.25, -6.75), seed=2)),
                                          "tests/hier_ref.py fast_sequence, shift (11.25, -6.75) per frame, seed 2")
        res["coding_slow"] = coding_bench(np.stack(subpel_ref.subpel_sequence(H, W, n, seed=2)),
                                          "tests/subpel_ref.py subpel_sequence, (1.25, 1.75) per frame, seed 2")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not res["search"]["condition_L2_S8_faster_than_plain_S32"]:
        sys.exit("L = 2, S = 8 is not faster than plain S = 32")


if __name__ == "__main__":
    main()

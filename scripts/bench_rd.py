"""Time the distortion kernel and the resident rate-distortion curve.

Kernel: vcf_distortion_u8 on 64 pairs of 4K RGB frames (3.19 GB read per launch, far more than the
256 MiB Infinity Cache), HIP events on the launch stream around N launches (default 20) after a
settling run past the clock ramp, median of R rounds.  Printed: ms per launch and the share of the
HBM roofline as in DESIGN.md §5 -- the bytes the kernel must move (two bytes per sample; the
records are a few KB) over the measured 6.3 TB/s copy rate, over the time.  The 2D-DCT encode
kernel (vcf_dct_dz_encode, one byte read and one written per sample) is timed the same way in the
same run, as the yardstick of what a streaming kernel of this library reaches on the box.

rd_curve: codec/rde.py rd_curve over 7 quantization steps on 16 synthetic 1080p frames, wall time
of the call (upload included), against the path through files it replaces, in the same run: per Q
and frame 2D-DCT encode_fn, decode_fn and RDE (evaluate) on the files.  Both give the same bytes
and RMSE (checked here).  The ratio is reported, not gated.

python scripts/bench_rd.py [N] [R] [--out profiles/rd_bench.json]
"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from vcf_amd import dct as D
from vcf_amd import distortion as DS
from vcf_amd import synthetic
from vcf_amd.codec import parser as P
from vcf_amd.codec import rde
from vcf_amd.codec.dct2d import CoDec
from vcf_amd.codec.eic import write_image
from vcf_amd.device import DeviceBuffer, Event, Stream, copy_dtod, set_device

HBM_BYTES_PER_S = 6.3e12         # measured copy rate (8.0 TB/s specified)
QS = [4, 8, 16, 32, 64, 96, 128]


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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def kernel_bench(n, rounds):
    N, H, W, C = 64, 2160, 3840, 3
    fb = H * W * C
    s = Stream()
    a, b, k = DeviceBuffer(N * fb), DeviceBuffer(N * fb), DeviceBuffer(N * fb)
    out = DeviceBuffer(N * C * DS.RECORD.itemsize)
    fa, fb2 = synthetic.synth_frame(H, W, 0), synthetic.synth_frame(H, W, 1)
    a.upload(fa, s)
    b.upload(fb2, s)
    for i in range(1, N):
        copy_dtod(a, i * fb, a, 0, fb, s)
        copy_dtod(b, i * fb, b, 0, fb, s)
    ms, lo, hi = timed(lambda: DS.sse_device(a, b, N, H, W, C, out, s), s, n, rounds)
    m = DS.records(out, N, C, H * W, s)
    d = fa.astype(np.int64) - fb2.astype(np.int64)
    assert (m.sse == (d * d).reshape(-1, C).sum(axis=0).astype(np.uint64)[None, :]).all(), "kernel result"
    moved = 2 * N * fb
    res = dict(frames=N, H=H, W=W, C=C, launches=n, rounds=rounds, ms_per_launch=ms, ms_min=lo, ms_max=hi,
               bytes_moved=moved, tb_per_s=moved / (ms * 1e-3) / 1e12,
               hbm_roofline_fraction=moved / HBM_BYTES_PER_S / (ms * 1e-3))
    ems, elo, ehi = timed(lambda: D.encode_device(a, N, H, W, 32, 0, out=k, stream=s), s, n, rounds)
    res["dct_encode_same_run"] = dict(ms_per_launch=ems, ms_min=elo, ms_max=ehi, bytes_moved=moved,
                                      hbm_roofline_fraction=moved / HBM_BYTES_PER_S / (ems * 1e-3))
    for buf in (a, b, k, out):
        buf.free()
    s.close()
    return res


def curve_bench():
    n, H, W = 16, 1080, 1920
    frames = np.stack([synthetic.synth_frame(H, W, 10 + i) for i in range(n)])
    rde.rd_curve(frames[:2], QS[:1])            # warm-up: code objects, the deflater's buffers
    t0 = time.perf_counter()
    curve = rde.rd_curve(frames, QS)
    t_resident = time.perf_counter() - t0
    with tempfile.TemporaryDirectory() as d:
        cwd = os.getcwd()
        os.chdir(d)                              # relative names: RDE's prefix rule cuts at the first dot
        try:
            for i in range(n):
                write_image(f"original_{i:04d}.png", frames[i])
            t0 = time.perf_counter()
            for c in curve:
                enc = CoDec(P.parse(P.dct_parser(), ["encode", "-q", str(c["Q"])]))
                dec = CoDec(P.parse(P.dct_parser(), ["decode", "-q", str(c["Q"])]))
                for i in range(n):
                    enc.encode_fn(f"original_{i:04d}.png", f"encoded_{i:04d}")
                    dec.decode_fn(f"encoded_{i:04d}", f"decoded_{i:04d}.png")
                    r = rde.evaluate(f"original_{i:04d}.png", f"encoded_{i:04d}", f"decoded_{i:04d}.png")
                    assert r.codestream_bytes == int(c["bytes"][i]) and r.rmse == c["rmse"][i], (c["Q"], i)
            t_files = time.perf_counter() - t0
        finally:
            os.chdir(cwd)
    return dict(frames=n, H=H, W=W, Qs=QS, rd_curve_s=t_resident, file_path_s=t_files, ratio=t_files / t_resident,
                curve=[dict(Q=c["Q"], bytes=float(c["bytes"].mean()), bpp=float(c["bpp"].mean()),
                            rmse=float(c["rmse"].mean()), psnr=float(c["psnr"].mean())) for c in curve])


def main():
    out_fn = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    argv = [a for a in sys.argv[1:] if not a.startswith("--") and a != out_fn]
    n = int(argv[0]) if len(argv) > 0 else 20
    rounds = int(argv[1]) if len(argv) > 1 else 5
    set_device(0)
    res = dict(kernel=kernel_bench(n, rounds))
    print(json.dumps(res["kernel"]), flush=True)
    res["rd_curve"] = curve_bench()
    if out_fn:
        os.makedirs(os.path.dirname(os.path.abspath(out_fn)), exist_ok=True)
        with open(out_fn, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

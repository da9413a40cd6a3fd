"""Time the deblocking kernel, its effect on the rate-distortion curve and its cost in decode_fns.

Kernel: vcf_deblock_u8 (B = 8, the default strengths of -q 32) on 64 blocky 4K RGB frames resident
in HBM (1.59 GB read and 1.59 GB written per launch, far more than the 256 MiB Infinity Cache), HIP
events on the launch stream around N launches (default 10) after a settling run past the clock
ramp, median of R rounds (default 5).  vcf_distortion_u8, which also streams two frame-sized
buffers, is timed the same way in the same run as the yardstick; the ratio is reported, not gated.

RD effect: codec/rde.py rd_curve (SSIM included) over -q 8, 16, 32, 64, 128 on 16 synthetic 1080p
frames (vcf_amd/synthetic.py) without the filter, with the default strengths and over the sweep
tc in {Q//16, Q//8, Q//4} x beta in {Q//2, Q, 2Q}.  The bytes are equal by construction, so RMSE and
SSIM compare at equal bytes.  tests/golden holds no natural images; the synthetic frames are all
this conclusion can rest on.

Decode cost: decode_fns of 16 x 1080p -B 8 files with and without -f deblock, wall time, same run.

python scripts/bench_deblock.py [N] [R] [--out profiles/deblock_bench.json]
"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from vcf_amd import deblock as DB
from vcf_amd import distortion as DS
from vcf_amd import synthetic
from vcf_amd.codec import parser as P
from vcf_amd.codec import rde
from vcf_amd.codec.dct2d import CoDec
from vcf_amd.codec.eic import write_image
from vcf_amd.device import DeviceBuffer, Event, Stream, copy_dtod, set_device

HBM_PEAK = 8.0e12                # specified
HBM_COPY = 6.3e12                # measured copy rate
QS = [8, 16, 32, 64, 128]


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
    N, H, W = 64, 2160, 3840
    fb = H * W * 3
    s = Stream()
    a, b = DeviceBuffer(N * fb), DeviceBuffer(N * fb)
    out = DeviceBuffer(N * 3 * DS.RECORD.itemsize)
    # a decoded frame: the synthetic one through the codec's quantizer at -q 32, so that lines are filtered
    from vcf_amd import dct as D
    f0 = D.decode(D.encode(synthetic.synth_frame(H, W, 0), 32), H, W, 32)
    a.upload(f0, s)
    for i in range(1, N):
        copy_dtod(a, i * fb, a, 0, fb, s)
    beta, tc = DB.default_strength(32)
    res = dict(frames=N, H=H, W=W, launches=n, rounds=rounds, bytes_moved=2 * N * fb)
    for B in (8, 4, 16):
        ms, lo, hi = timed(lambda: DB.deblock_device(a, N, H, W, B, 0, 0, beta, tc, out=b, stream=s), s, n, rounds)
        res[f"deblock_B{B}"] = dict(ms_per_launch=ms, ms_min=lo, ms_max=hi, tb_per_s=2 * N * fb / (ms * 1e-3) / 1e12,
                                    share_of_8tb=2 * N * fb / HBM_PEAK / (ms * 1e-3),
                                    share_of_copy_rate=2 * N * fb / HBM_COPY / (ms * 1e-3))
    dms, dlo, dhi = timed(lambda: DS.sse_device(a, b, N, H, W, 3, out, s), s, n, rounds)
    res["distortion_same_run"] = dict(ms_per_launch=dms, ms_min=dlo, ms_max=dhi,
                                      tb_per_s=2 * N * fb / (dms * 1e-3) / 1e12,
                                      share_of_8tb=2 * N * fb / HBM_PEAK / (dms * 1e-3))
    res["deblock_over_distortion"] = res["deblock_B8"]["ms_per_launch"] / dms
    for buf in (a, b, out):
        buf.free()
    s.close()
    return res


def _mean(curve, key):
    return [float(np.mean(c[key])) for c in curve]


def rd_bench():
    n, H, W = 16, 1080, 1920
    frames = np.stack([synthetic.synth_frame(H, W, 10 + i) for i in range(n)])
    plain = rde.rd_curve(frames, QS, ssim=True)
    res = dict(frames=n, H=H, W=W, Qs=QS, source="vcf_amd/synthetic.py synth_frame, seeds 10..25",
               bytes=_mean(plain, "bytes"), plain=dict(rmse=_mean(plain, "rmse"), ssim=_mean(plain, "ssim")))
    d = rde.rd_curve(frames, QS, ssim=True, filter="deblock")
    assert all(np.array_equal(p["bytes"], c["bytes"]) for p, c in zip(plain, d))
    res["default"] = dict(rule="beta = Q, tc = max(1, Q // 8)", rmse=_mean(d, "rmse"), ssim=_mean(d, "ssim"))
    sweep = []
    for Q, p in zip(QS, plain):
        for tc in sorted({max(1, Q // 16), max(1, Q // 8), max(1, Q // 4)}):
            for beta in (Q // 2, Q, 2 * Q):
                c = rde.rd_curve(frames, [Q], ssim=True, filter="deblock", deblock_beta=beta, deblock_tc=tc)[0]
                sweep.append(dict(Q=Q, beta=beta, tc=tc, rmse=float(c["rmse"].mean()), ssim=float(c["ssim"].mean()),
                                  d_rmse=float(c["rmse"].mean() - p["rmse"].mean()),
                                  d_ssim=float(c["ssim"].mean() - p["ssim"].mean())))
    res["sweep"] = sweep
    return res


def decode_bench():
    n, H, W = 16, 1080, 1920
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for i in range(n):
            write_image(os.path.join(d, f"o_{i:04d}.png"), synthetic.synth_frame(H, W, 10 + i))
        enc = CoDec(P.parse(P.dct_parser(), ["encode", "-q", "32"]))
        enc.encode_fns([(os.path.join(d, f"o_{i:04d}.png"), os.path.join(d, f"e_{i:04d}")) for i in range(n)])
        pairs = [(os.path.join(d, f"e_{i:04d}"), os.path.join(d, f"d_{i:04d}.png")) for i in range(n)]
        for name, argv, kw in (("no_filter", ["decode", "-q", "32"], {}),
                               ("deblock", ["decode", "-q", "32", "-f", "deblock"], dict(filter="deblock"))):
            dec = CoDec(P.parse(P.dct_parser(**kw), argv))
            dec.decode_fns(pairs)                      # warm-up: code objects, buffers
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                dec.decode_fns(pairs)
                ts.append(time.perf_counter() - t0)
            out[name] = dict(s_median=float(np.median(ts)), s_min=min(ts), s_max=max(ts), runs=5)
    out["frames"], out["H"], out["W"] = n, H, W
    out["ratio"] = out["deblock"]["s_median"] / out["no_filter"]["s_median"]
    return out


def main():
    out_fn = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    argv = [a for a in sys.argv[1:] if not a.startswith("--") and a != out_fn]
    n = int(argv[0]) if len(argv) > 0 else 10
    rounds = int(argv[1]) if len(argv) > 1 else 5
    set_device(0)
    res = dict(kernel=kernel_bench(n, rounds))
    print(json.dumps(res["kernel"]), flush=True)
    res["decode_fns"] = decode_bench()
    print(json.dumps(res["decode_fns"]), flush=True)
    res["rd"] = rd_bench()
    if out_fn:
        os.makedirs(os.path.dirname(os.path.abspath(out_fn)), exist_ok=True)
        with open(out_fn, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

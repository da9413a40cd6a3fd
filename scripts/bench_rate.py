"""Time the index-histogram kernel and the rate control built on it.

Kernel: vcf_index_hist_u8 on 64 index frames of 4K (one synthetic frame through the DCT encode at
Q = 32, copied 64 times), whole plane and 8 x 8 subband grid, timed as scripts/bench_rd.py times the
distortion kernel (HIP events around N launches after a settling run, median of R rounds), with
vcf_distortion_u8 on buffers of the same size in the same run as the yardstick.  The HBM bound is
one read of the indices over the measured 6.3 TB/s copy rate.

choose_q: 16 synthetic 1080p frames at a budget of 1 bit per pixel, wall time of the call from host
frames (upload included): rate = "estimate" and rate = "coded" with -c TIFF, rate = "coded" with
-c TCBAACP; and the comparison the acceptance line names: the same bisection driven from the host
through rde.rd_curve, one call per probed Q (each uploads the frames and brings back sizes and
distortion, as a loop over RD-curve.py does).  The variants alternate, median of three each.

Estimate quality: rate.estimate_bytes(..., "subband") over the real code-stream bytes of -c TIFF and
-c TCBAAC2D, on the 64 x 96 frames of tests/test_rate_gpu.py and on the 1080p frames.

python scripts/bench_rate.py [N] [R] [--out profiles/rate_bench.json]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from bench_rd import HBM_BYTES_PER_S, timed
from vcf_amd import dct as D
from vcf_amd import distortion as DS
from vcf_amd import rate as R
from vcf_amd import synthetic
from vcf_amd.codec import parser as P
from vcf_amd.codec import ratecontrol as RC
from vcf_amd.codec import rde
from vcf_amd.codec.dct2d import CoDec
from vcf_amd.device import DeviceBuffer, Stream, copy_dtod, set_device


def codec(entropy="TIFF"):
    return CoDec(P.parse(P.dct_parser(entropy=entropy), ["encode", "-c", entropy]))


def kernel_bench(n, rounds):
    N, H, W = 64, 2160, 3840
    fb = H * W * 3
    s = Stream()
    k = DeviceBuffer(N * fb)
    frame = synthetic.synth_frame(H, W, 0)
    idx = D.encode(frame, 32)
    k.upload(idx, s)
    for i in range(1, N):
        copy_dtod(k, i * fb, k, 0, fb, s)
    res = dict(frames=N, H=H, W=W, Q=32, launches=n, rounds=rounds, bytes_moved=N * fb,
               hbm_bound_ms=N * fb / HBM_BYTES_PER_S * 1e3, zero_index_share=float((idx == 128).mean()))
    for name, grid in (("plane", (1, 1)), ("subbands_8x8", (8, 8))):
        out = DeviceBuffer(N * grid[0] * grid[1] * 768 * 4)
        ms, lo, hi = timed(lambda: R.histogram_device(k, (N, H, W, 3), grid, out, s), s, n, rounds)
        got = out.download(np.empty((N, grid[0] * grid[1], 3, 256), np.uint32))
        rh, cw = H // grid[0], W // grid[1]
        want = np.stack([np.bincount(idx[i * rh:(i + 1) * rh, j * cw:(j + 1) * cw, c].ravel(), minlength=256)
                         for i in range(grid[0]) for j in range(grid[1]) for c in range(3)]).reshape(got.shape[1:])
        assert all(np.array_equal(got[f], want) for f in (0, N - 1)), "counts differ from np.bincount"
        res[name] = dict(ms_per_launch=ms, ms_min=lo, ms_max=hi, hbm_roofline_fraction=res["hbm_bound_ms"] / ms)
        out.free()
    b = DeviceBuffer(N * fb)
    copy_dtod(b, 0, k, 0, N * fb, s)
    dout = DeviceBuffer(N * 3 * DS.RECORD.itemsize)
    dms, dlo, dhi = timed(lambda: DS.sse_device(k, b, N, H, W, 3, dout, s), s, n, rounds)
    res["distortion_same_run"] = dict(ms_per_launch=dms, ms_min=dlo, ms_max=dhi, bytes_moved=2 * N * fb,
                                      hbm_roofline_fraction=2 * res["hbm_bound_ms"] / dms)
    for buf in (k, b, dout):
        buf.free()
    s.close()
    return res


def host_loop(frames, budget, q_min=1, q_max=2048):
    """The bisection of ratecontrol.bisect_q with rde.rd_curve as the probe: one call per distinct Q of a step."""
    def rate_fn(q, active):
        sizes = np.zeros(len(q), np.int64)
        for Q in sorted(set(q[active].tolist())):
            sizes[q == Q] = rde.rd_curve(frames, [Q])[0]["bytes"][q == Q]
        return sizes
    return RC.bisect_q(rate_fn, budget, q_min, q_max)


def choose_bench():
    n, H, W, bpp = 16, 1080, 1920, 1.0
    frames = np.stack([synthetic.synth_frame(H, W, 10 + i) for i in range(n)])
    budget = RC.budgets_of(n, H, W, target_bpp=bpp)
    tiff, tcp = codec("TIFF"), codec("TCBAACP")
    runs = {
        "estimate_tiff": lambda: RC.choose_q_frames(frames, target_bpp=bpp, codec=tiff, rate="estimate"),
        "coded_tiff": lambda: RC.choose_q_frames(frames, target_bpp=bpp, codec=tiff, rate="coded"),
        "coded_tcbaacp": lambda: RC.choose_q_frames(frames, target_bpp=bpp, codec=tcp, rate="coded"),
        "host_loop_rd_curve": lambda: host_loop(frames, budget),
    }
    RC.choose_q_frames(frames[:2], target_bpp=bpp, codec=tiff, rate="estimate", q_max=64)   # warm-up: code objects,
    RC.choose_q_frames(frames[:2], target_bpp=bpp, codec=tcp, rate="coded", q_max=64)       # the coders' buffers
    rde.rd_curve(frames[:2], [32])
    t, last = {k: [] for k in runs}, {}
    for _ in range(3):
        for name, fn in runs.items():
            t0 = time.perf_counter()
            last[name] = fn()
            t[name].append(time.perf_counter() - t0)
    res = dict(frames=n, H=H, W=W, target_bpp=bpp, budget_bytes=int(budget[0]), runs=t)
    for name in runs:
        res[name + "_s"] = float(np.median(t[name]))
    for name in ("estimate_tiff", "coded_tiff", "coded_tcbaacp"):
        c = last[name]
        res[name] = dict(q=c.q.tolist(), bytes=c.bytes.tolist(), met=c.met.tolist(), probes=c.probes,
                         corrections=c.corrections, rmse=np.round(c.rmse, 4).tolist())
    hq, hmet, hbytes, hsteps = last["host_loop_rd_curve"]
    res["host_loop_rd_curve"] = dict(q=hq.tolist(), bytes=hbytes.tolist(), met=hmet.tolist(), probes=hsteps)
    res["host_loop_reaches_coded_q"] = bool(np.array_equal(hq, last["coded_tiff"].q))
    res["estimate_over_host_loop"] = res["estimate_tiff_s"] / res["host_loop_rd_curve_s"]
    res["estimate_beats_host_loop"] = bool(res["estimate_tiff_s"] < res["host_loop_rd_curve_s"])
    return res, frames


def estimate_quality(frames_1080p):
    """estimate_bytes("subband") / coded bytes per frame, at the Q the coded search chooses for 1 bit per pixel."""
    out = {}
    small = np.stack([synthetic.synth_frame(64, 96, seed) for seed in (1, 2, 3)])
    for label, frames in (("64x96", small), ("1080p", frames_1080p[:4])):
        for entropy in ("TIFF", "TCBAAC2D"):
            c = RC.choose_q_frames(frames, target_bpp=1.0, codec=codec(entropy), rate="coded")
            est = []
            for f, q in zip(frames, c.q):
                k = D.encode(f, int(q))
                est.append(int(R.estimate_bytes(R.histogram(k[None], regions=(8, 8)), "subband")[0]) + RC.SIDE_BYTES)
            out[f"{label}_{entropy}"] = dict(q=c.q.tolist(), coded_bytes=c.bytes.tolist(), estimate_bytes=est,
                                             estimate_over_coded=(np.array(est) / c.bytes).round(4).tolist())
    return out


def main():
    set_device(0)
    out_fn = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    argv = [a for a in sys.argv[1:] if not a.startswith("--") and a != out_fn]
    n = int(argv[0]) if len(argv) > 0 else 10
    rounds = int(argv[1]) if len(argv) > 1 else 5
    res = dict(kernel=kernel_bench(n, rounds))
    print(json.dumps(res["kernel"]), flush=True)
    res["choose_q"], frames = choose_bench()
    print(json.dumps({k: v for k, v in res["choose_q"].items() if k.endswith("_s") or k.startswith("estimate_")}),
          flush=True)
    res["estimate_quality"] = estimate_quality(frames)
    if out_fn:
        os.makedirs(os.path.dirname(os.path.abspath(out_fn)), exist_ok=True)
        with open(out_fn, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

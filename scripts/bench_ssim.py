"""Time the SSIM kernel and the resident rate-distortion curve with it.

Kernel: vcf_ssim_u8 on 64 pairs of 4K RGB frames, timed as scripts/bench_rd.py times the distortion
kernel (HIP events around N launches after a settling run, median of R rounds), and
vcf_distortion_u8 on the same buffers in the same run as the yardstick: both read the same two
bytes per sample.  Printed: ms per launch, the HBM bound (two reads of 3 bytes per pixel over the
measured 6.3 TB/s copy rate) and the share of it the kernel reaches, windows per second, and what the
compiler reports for the kernel's code object (registers, LDS, waves per SIMD: hipcc's
kernel-resource-usage remarks for vcf_ssim.hip under the library's own flags).  The records of the
timed buffers are checked against tests/ssim_ref.py on a crop.

rd_curve: codec/rde.py rd_curve over 7 quantization steps on 16 synthetic 1080p frames, wall time of
the call (upload included) with and without ssim=True, alternating, median of three each.

python scripts/bench_ssim.py [N] [R] [--out profiles/ssim_bench.json]
python scripts/bench_ssim.py --once K      K launches on 8 frame pairs and nothing else (counter passes)
"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from bench_rd import HBM_BYTES_PER_S, QS, timed
from vcf_amd import _build
from vcf_amd import distortion as DS
from vcf_amd import synthetic
from vcf_amd._lib import lib
from vcf_amd.codec import rde
from vcf_amd.device import DeviceBuffer, Stream, copy_dtod, set_device

H, W, C = 2160, 3840, 3


def kernel_resources():
    """{kernel: {vgprs, sgprs, lds_bytes, scratch_bytes, waves_per_simd}} from the compiler's remarks."""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([_build.hipcc(), *_build._flags(), "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(_build.CSRC, "vcf_ssim.hip"), "-o", os.path.join(d, "ssim.o")],
                           capture_output=True, text=True, timeout=300)
    res, cur = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "LDS Size [bytes/block]": "lds_bytes",
            "ScratchSize [bytes/lane]": "scratch_bytes", "Occupancy [waves/SIMD]": "waves_per_simd"}
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            t = re.search(r"(ssim_\w*?kernel)(?:ILi(\d+)E)?", m.group(1))
            cur = res.setdefault(t.group(1) + (f"<{t.group(2)}>" if t.group(2) else "") if t else m.group(1), {})
            continue
        m = re.search(r"remark:(?: \S+:\d+:\d+:)? +([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return res


def buffers(N, s):
    fb = H * W * C
    a, b = DeviceBuffer(N * fb), DeviceBuffer(N * fb)
    fa, fb2 = synthetic.synth_frame(H, W, 0), synthetic.synth_frame(H, W, 1)
    a.upload(fa, s)
    b.upload(fb2, s)
    for i in range(1, N):
        copy_dtod(a, i * fb, a, 0, fb, s)
        copy_dtod(b, i * fb, b, 0, fb, s)
    return a, b, fa, fb2


def kernel_bench(n, rounds):
    import ssim_ref as R
    N, fb = 64, H * W * C
    s = Stream()
    a, b, fa, fb2 = buffers(N, s)
    out = DeviceBuffer(N * C * DS.SSIM_RECORD.itemsize)
    dout = DeviceBuffer(N * C * DS.RECORD.itemsize)
    ms, lo, hi = timed(lambda: DS.ssim_device(a, b, N, H, W, C, out, s), s, n, rounds)
    m = DS.ssim_records(out, N, C, s)
    assert (m.sum_k == m.sum_k[0]).all() and (m.min_k == m.min_k[0]).all(), "equal frames, equal records"
    # the restatement on the whole 4K frame takes seconds on the host: do it once
    want = R.ssim_ref(fa, fb2)
    assert np.array_equal(m.sum_k[0], want[0][0]) and m.windows == want[1] and np.array_equal(m.min_k[0], want[2][0])
    dms, dlo, dhi = timed(lambda: DS.sse_device(a, b, N, H, W, C, dout, s), s, n, rounds)
    moved = 2 * N * fb
    bound_ms = moved / HBM_BYTES_PER_S * 1e3
    windows = N * C * (H - 10) * (W - 10)
    res = dict(frames=N, H=H, W=W, C=C, launches=n, rounds=rounds, tile=int(lib().vcf_ssim_tile()),
               ms_per_launch=ms, ms_min=lo, ms_max=hi, bytes_moved=moved, hbm_bound_ms=bound_ms,
               hbm_roofline_fraction=bound_ms / ms, windows=windows, gwindows_per_s=windows / (ms * 1e-3) / 1e9,
               ssim_per_channel=m.per_channel()[0].tolist(),
               distortion_same_run=dict(ms_per_launch=dms, ms_min=dlo, ms_max=dhi, hbm_roofline_fraction=bound_ms / dms),
               ratio_to_distortion=ms / dms)
    for buf in (a, b, out, dout):
        buf.free()
    s.close()
    return res


def curve_bench():
    n, h, w = 16, 1080, 1920
    frames = np.stack([synthetic.synth_frame(h, w, 10 + i) for i in range(n)])
    rde.rd_curve(frames[:2], QS[:1], ssim=True)          # warm-up: code objects, the deflater's buffers
    t = {False: [], True: []}
    for _ in range(3):
        for flag in (False, True):
            t0 = time.perf_counter()
            curve = rde.rd_curve(frames, QS, ssim=flag)
            t[flag].append(time.perf_counter() - t0)
    plain, with_ssim = float(np.median(t[False])), float(np.median(t[True]))
    return dict(frames=n, H=h, W=w, Qs=QS, rd_curve_s=plain, rd_curve_ssim_s=with_ssim, added_s=with_ssim - plain,
                runs=dict(plain=t[False], ssim=t[True]),
                curve=[dict(Q=c["Q"], bpp=float(c["bpp"].mean()), rmse=float(c["rmse"].mean()),
                            psnr=float(c["psnr"].mean()), ssim=float(c["ssim"].mean())) for c in curve])


def once(k):
    s = Stream()
    a, b, _, _ = buffers(8, s)
    out = DeviceBuffer(8 * C * DS.SSIM_RECORD.itemsize)
    for _ in range(k):
        DS.ssim_device(a, b, 8, H, W, C, out, s)
    s.synchronize()
    print("ok", k)


def main():
    set_device(0)
    if "--once" in sys.argv:
        return once(int(sys.argv[sys.argv.index("--once") + 1]))
    out_fn = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    argv = [a for a in sys.argv[1:] if not a.startswith("--") and a != out_fn]
    n = int(argv[0]) if len(argv) > 0 else 10
    rounds = int(argv[1]) if len(argv) > 1 else 5
    res = dict(kernel=kernel_bench(n, rounds))
    print(json.dumps(res["kernel"]), flush=True)
    res["code_object"] = kernel_resources()
    res["rd_curve"] = curve_bench()
    if out_fn:
        os.makedirs(os.path.dirname(os.path.abspath(out_fn)), exist_ok=True)
        with open(out_fn, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

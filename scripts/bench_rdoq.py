#!/usr/bin/env python3
"""RDOQ on one MI355X -> profiles/rdoq_bench.json.

Kernel: vcf_dct_dz_encode_rdoq against vcf_dct_dz_encode on the same buffers (64 x 4K frames, Q = 32,
mu = 0.2), HIP events around 10 launches after a settling launch, the two kernels alternating, median
of 5 rounds; S-smooth frames (nearly every index zero) and uniform-random ones (nearly every index a
candidate).  The timed output is checked against tests/rdoq_ref.py on the first and last frame.
Pipeline: the stages of rdoq.encode_frames_device, wall clock around synchronised steps.
Gain: 16 x 1080p S-smooth frames, mu x Q, bytes under -c TIFF and -c TCBAAC2D, RMSE and SSIM from
rd_curve, and per codec the bytes at the plain curve's RMSE (log-linear interpolation of the plain curve).

    python scripts/bench_rdoq.py [--frames 64] [--gain-frames 16] [--out profiles/rdoq_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from vcf_amd import dct as D, rate, rdoq as R  # noqa: E402
from vcf_amd.device import DeviceBuffer, Event, synchronize  # noqa: E402
from vcf_amd.synthetic import synth_frame  # noqa: E402

LAUNCHES, ROUNDS = 10, 5


def timed(fn):
    fn()
    a, b = Event(), Event()
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_ms(b) / LAUNCHES


def kernel_times(frames, Q, mu, check):
    import rdoq_ref as RR
    n, H, W, _ = frames.shape
    Hp, Wp = D.padded_shape(H, W)
    lam = R.lambda_of(mu, Q)
    src, k = DeviceBuffer.from_array(frames), DeviceBuffer(n * Hp * Wp * 3)
    D.encode_device(src, n, H, W, Q, out=k)
    counts = rate.histogram(k, (n, Hp, Wp, 3), (8, 8))
    bits = R.cost_table(counts)
    tab = DeviceBuffer.from_array(bits)
    plain = lambda: D.encode_device(src, n, H, W, Q, out=k)                        # noqa: E731
    rdoq = lambda: R.encode_device(src, n, H, W, Q, lam, tab, n, out=k)            # noqa: E731
    t = {"plain": [], "rdoq": []}
    for _ in range(ROUNDS):
        t["plain"].append(timed(plain))
        t["rdoq"].append(timed(rdoq))
    synchronize()
    for f in check:
        got = k.download(np.empty((Hp, Wp, 3), np.uint8), offset=f * Hp * Wp * 3)
        assert np.array_equal(got, RR.encode_frame(frames[f], Q, lam, bits[f])), f"frame {f} differs from rdoq_ref"
    nz = float(1.0 - counts[:, :, :, 128].sum() / (n * Hp * Wp * 3))
    for b in (src, k, tab):
        b.free()
    p, r = float(np.median(t["plain"])), float(np.median(t["rdoq"]))
    return dict(frames=n, H=H, W=W, Q=Q, mu=mu, plain_ms=p, rdoq_ms=r, ratio=r / p, rounds=t,
                nonzero_index_fraction=nz, checked_frames=list(check))


def pipeline_times(frames, Q, mu):
    n, H, W, _ = frames.shape
    Hp, Wp = D.padded_shape(H, W)
    lam = R.lambda_of(mu, Q)
    src, k = DeviceBuffer.from_array(frames), DeviceBuffer(n * Hp * Wp * 3)
    counts = np.empty((n, 64, 3, 256), np.uint32)
    hist = rate.histogram_device(k, (n, Hp, Wp, 3), (8, 8))
    tab = DeviceBuffer(counts.size * 8)
    out = {}

    def stage(name, fn):
        synchronize()
        t0 = time.perf_counter()
        res = fn()
        synchronize()
        out.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
        return res

    for _ in range(ROUNDS + 1):
        stage("plain_pass", lambda: D.encode_device(src, n, H, W, Q, out=k))
        stage("histogram", lambda: rate.histogram_device(k, (n, Hp, Wp, 3), (8, 8), out=hist))
        stage("download", lambda: hist.download(counts))
        bits = stage("cost_table", lambda: R.cost_table(counts))
        stage("upload", lambda: tab.upload(bits))
        stage("rdoq_pass", lambda: R.encode_device(src, n, H, W, Q, lam, tab, n, out=k))
    for b in (src, k, hist, tab):
        b.free()
    med = {name + "_ms": float(np.median(v[1:])) for name, v in out.items()}     # the first round settles
    med["total_ms"] = float(sum(med.values()))
    return dict(frames=n, H=H, W=W, Q=Q, mu=mu, **med)


def gain(frames, Qs, mus):
    from vcf_amd.codec.entropy import make_entropy
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.rde import rd_curve
    n, H, W, _ = frames.shape
    coder = make_entropy(P.parse(P.dct_parser(entropy="TCBAAC2D"), ["encode", "-c", "TCBAAC2D"]))
    rows = []
    for mu in mus:
        curve = rd_curve(frames, Qs, ssim=True, rdoq=None if mu == 0 else mu)
        for c in curve:
            Q = c["Q"]
            idx = D.encode(frames, Q) if mu == 0 else R.encode(frames, Q, R.lambda_of(mu, Q))
            tcb = 0
            for f in range(n):
                cs = coder.compress(idx[f])
                cs.seek(0)
                tcb += len(cs.read()) + 12
            rows.append(dict(mu=mu, Q=Q, tiff_bytes=float(c["bytes"].sum()), tcbaac2d_bytes=float(tcb),
                             rmse=float(c["rmse"].mean()), ssim=float(c["ssim"].mean())))
    # bytes of the plain curve at each RDOQ point's RMSE (log bytes linear in RMSE between the plain points)
    plain = sorted((r for r in rows if r["mu"] == 0), key=lambda r: r["rmse"])
    for r in rows:
        for key in ("tiff_bytes", "tcbaac2d_bytes"):
            xs, ys = [p["rmse"] for p in plain], [np.log(p[key]) for p in plain]
            inside = xs[0] <= r["rmse"] <= xs[-1]
            r["plain_" + key + "_at_equal_rmse"] = float(np.exp(np.interp(r["rmse"], xs, ys))) if inside else None
            ref = r["plain_" + key + "_at_equal_rmse"]
            r[key.replace("_bytes", "") + "_saving_at_equal_rmse"] = None if ref is None else 1.0 - r[key] / ref
    best = {}
    for key in ("tiff", "tcbaac2d"):
        wins = [r for r in rows if r["mu"] > 0 and (r[key + "_saving_at_equal_rmse"] or 0) > 0]
        best[key] = max(wins, key=lambda r: r[key + "_saving_at_equal_rmse"]) if wins else "no mu wins"
    return dict(frames=n, H=H, W=W, rows=rows, best=best)


def kernel_resources():
    """hipcc's kernel-resource-usage remarks for every instantiation of the RDOQ kernel and of the plain
    encode kernel, from a compile of the two sources with the library's own flags (host work: no GPU)."""
    import re
    import subprocess
    import tempfile
    from vcf_amd import _build
    fields = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes",
              "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes",
              "VGPRs Spill": "vgpr_spills", "SGPRs Spill": "sgpr_spills"}
    names = {"dct_dz_encode_rdoq_kernel": ("pow2", "subbands", "byte_loads"),
             "dct_dz_encode_kernel": ("pow2", "subbands", "perceptual", "byte_loads", "packed")}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src in ("vcf_dct_rdoq.hip", "vcf_dct_dz.hip"):
            cmd = [_build.hipcc(), *_build._flags(), "-Rpass-analysis=kernel-resource-usage", "-c",
                   os.path.join(_build.CSRC, src), "-o", os.path.join(tmp, "a.o")]
            log = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
            cur = None
            for line in log.splitlines():
                m = re.search(r"remark: +Function Name: (\S+)", line)
                if m:
                    cur = None
                    for kernel, flags in names.items():
                        t = re.search(r"\d+" + kernel + r"I((?:Lb[01]E)+)", m.group(1))
                        if t:
                            bits = re.findall(r"Lb([01])E", t.group(1))
                            on = [f for f, b in zip(flags, bits) if b == "1"]
                            cur = out.setdefault(f"{kernel}<{', '.join(on) or 'general Q, -x'}>", {})
                    continue
                m = re.search(r"remark: +([A-Za-z][^:]*): (\d+)", line)
                if m and cur is not None and m.group(1).strip() in fields:
                    cur[fields[m.group(1).strip()]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--gain-frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rdoq_bench.json"))
    a = ap.parse_args()
    H, W = 2160, 3840
    base = [synth_frame(H, W, s) for s in range(4)]
    smooth = np.stack([base[i % 4] for i in range(a.frames)])
    noise = np.random.Generator(np.random.PCG64(1)).integers(0, 256, (a.frames, H, W, 3), dtype=np.uint8)
    res = {"launches": LAUNCHES, "rounds": ROUNDS}

    def save():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    res["kernel_smooth"] = kernel_times(smooth, 32, 0.2, (0, a.frames - 1))
    print(json.dumps({k: v for k, v in res["kernel_smooth"].items() if k != "rounds"}), flush=True)
    res["kernel_random"] = kernel_times(noise, 32, 0.2, (0, a.frames - 1))
    print(json.dumps({k: v for k, v in res["kernel_random"].items() if k != "rounds"}), flush=True)
    del noise
    save()
    res["pipeline_smooth"] = pipeline_times(smooth, 32, 0.2)
    print(json.dumps(res["pipeline_smooth"]), flush=True)
    del smooth
    save()
    g = np.stack([synth_frame(1080, 1920, 10 + s) for s in range(a.gain_frames)])
    res["gain"] = gain(g, [8, 16, 32, 64], [0, 0.05, 0.1, 0.2, 0.4])
    print(json.dumps(res["gain"]["best"]), flush=True)
    res["resources"] = kernel_resources()
    save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()

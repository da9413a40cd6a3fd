"""Time the 2D-KLT kernels: 64 4K frames per launch, B = 8 and B = 16, Q = 32.
HIP events on the launch stream around N launches (default 20) after a
settling run past the clock ramp; median of R rounds.  Moments, encode and
decode are timed separately, each frame with its own trained basis.

Printed per case: ms per launch, the HBM roofline fraction (the bytes the
algorithm needs: u8 RGB frame + u8 coefficient frame, about 6 B/pixel, the
moments the RGB frame alone, over the measured 6.3 TB/s copy rate), and the
float64 issue rate: the dense transform's D multiply-adds per coefficient
(2 D flops; idle lanes and the float32 -> float64 widening on decode not
counted) against the 78.6 TFLOP/s FP64 vector peak of the MI355X's public
specification.  The moments are integer work (D (D + 1) / 2 multiply-adds per
block and channel); for them the integer rate is printed in the same unit.
Next to the kernels, the host training time: numpy.linalg.eigh of one frame's
three D x D covariance matrices, per frame.  For orientation, the DCT encode
and decode per-launch times at the same frames and B = 8 on the same box.

python scripts/bench_klt.py [N] [R] [--out profiles/klt_bench.json]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from vcf_amd import synthetic
import vcf_amd.dct as D
import vcf_amd.klt as K
from vcf_amd.device import DeviceBuffer, Event, Stream, set_device

HBM_BYTES_PER_S = 6.3e12      # measured copy rate (8.0 TB/s specified)
FP64_FMA_PER_S = 78.6e12 / 2  # FP64 vector peak of the public specification, as multiply-adds


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


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(argv[0]) if len(argv) > 0 else 20
    rounds = int(argv[1]) if len(argv) > 1 else 5
    out_fn = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    set_device(0)
    H, W, F, Q = 2160, 3840, 64, 32
    base = np.stack([synthetic.synth_frame(H, W, s) for s in range(4)])
    frames = np.concatenate([base] * (F // 4))
    din = DeviceBuffer.from_array(frames)
    drgb = DeviceBuffer(F * H * W * 3)
    s = Stream()
    res = dict(frames=F, H=H, W=W, Q=Q, launches=n, rounds=rounds, cases=[])
    for B in (8, 16):
        Dd = B * B
        Hp, Wp = K.padded_shape(H, W, B)[:2]
        N = (Hp // B) * (Wp // B)
        # the bases of the four distinct frames: moments on the GPU, eigh on the host (timed)
        S1, S2 = K._moments(din, 4, H, W, B)
        C = K.covariance(S1, S2, N)
        t0 = time.perf_counter()
        w4 = np.stack([np.stack([K.basis(C[i, c]) for c in range(3)]) for i in range(4)])
        eigh_ms = (time.perf_counter() - t0) * 1e3 / 4
        res["cases"].append(dict(step="host eigh, per frame (3 channels)", B=B, D=Dd, ms=round(eigh_ms, 3)))
        print(json.dumps(res["cases"][-1]), flush=True)
        w64 = np.concatenate([w4] * (F // 4))
        dw64 = DeviceBuffer.from_array(w64)
        dw32 = DeviceBuffer.from_array(w64.astype(np.float32))
        dk = DeviceBuffer(F * Hp * Wp * 3)
        d1, d2 = DeviceBuffer(F * 3 * Dd * 8), DeviceBuffer(F * 3 * Dd * Dd * 8)
        mom = lambda: K.moments_device(din, F, H, W, B, d1, d2, stream=s)  # noqa: E731
        enc = lambda: K.encode_device(din, F, H, W, dw64, Q, 0, out=dk, stream=s, block_size=B)  # noqa: E731
        dec = lambda: K.decode_device(dk, F, H, W, dw32, Q, 0, out=drgb, stream=s, block_size=B)  # noqa: E731
        coef = F * Hp * Wp * 3
        work = dict(moments=(F * H * W * 3, F * 3 * N * Dd * (Dd + 1) // 2),
                    encode=(F * H * W * 3 + coef, coef * Dd), decode=(F * H * W * 3 + coef, coef * Dd))
        for name, fn in (("moments", mom), ("encode", enc), ("decode", dec)):
            med, lo, hi = timed(fn, s, n, rounds)
            hbm, fma = work[name]
            rate = "int_mad_vs_fp64_issue_fraction" if name == "moments" else "fp64_issue_fraction"
            res["cases"].append({
                "kernel": f"klt_{name}", "B": B, "D": Dd, "ms": round(med, 4), "ms_min": round(lo, 4),
                "ms_max": round(hi, 4), "hbm_bytes": hbm,
                "hbm_roofline_fraction": round(hbm / HBM_BYTES_PER_S / (med * 1e-3), 4), "multiply_adds": fma,
                rate: round(fma / FP64_FMA_PER_S / (med * 1e-3), 4),
                "gpixel_per_s": round(F * H * W / (med * 1e-3) / 1e9, 2)})
            print(json.dumps(res["cases"][-1]), flush=True)
        for b in (dw64, dw32, dk, d1, d2):
            b.free()
    Hp, Wp = D.padded_shape(H, W, 8)
    dk = DeviceBuffer(F * Hp * Wp * 3)
    for name, fn in (("encode", lambda: D.encode_device(din, F, H, W, Q, 0, out=dk, stream=s)),
                     ("decode", lambda: D.decode_device(dk, F, H, W, Q, 0, out=drgb, stream=s))):
        med, lo, hi = timed(fn, s, n, rounds)
        res["cases"].append(dict(kernel=f"dct_{name} (orientation)", B=8, ms=round(med, 4), ms_min=round(lo, 4),
                                 ms_max=round(hi, 4)))
        print(json.dumps(res["cases"][-1]), flush=True)
    if out_fn:
        os.makedirs(os.path.dirname(os.path.abspath(out_fn)), exist_ok=True)
        with open(out_fn, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

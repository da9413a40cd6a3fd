"""Time the lapped 2D-MDCT encode and decode kernels: 64 4K frames per launch,
B = 8 and B = 32, Q = 32.  HIP events on the launch stream around N launches
(default 100) after a settling run past the clock ramp; median of R rounds.

Printed per case: ms per launch, the HBM roofline fraction (the bytes the
algorithm needs: u8 RGB frame + u8 padded coefficient frame, about 6 B/pixel
plus the pad, over the measured 6.3 TB/s copy rate), and the float64 issue
rate: the direct form's 2 * 2N multiply-adds per coefficient (halo and idle
lanes not counted) against the 78.6 TFLOP/s FP64 vector peak of the
MI355X's public specification.  For orientation, the DCT encode and decode
per-launch times at the same frames and B = 8 on the same box.

python scripts/bench_mdct.py [N] [R] [--out profiles/mdct_bench.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from vcf_amd import synthetic
import vcf_amd.dct as D
import vcf_amd.mdct as M
from vcf_amd.device import DeviceBuffer, Event, Stream, set_device

HBM_BYTES_PER_S = 6.3e12      # measured copy rate (8.0 TB/s specified)
FP64_FMA_PER_S = 78.6e12 / 2  # FP64 vector peak of the public specification, as multiply-adds


def timed(fn, s, n, rounds, settle_s=1.0):
    import time
    t0 = time.time()
    while time.time() - t0 < settle_s:   # past the clock ramp
        for _ in range(5):
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
    n = int(argv[0]) if len(argv) > 0 else 100
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
    for B in (8, 32):
        Hp, Wp = M.padded_shape(H, W, B)[:2]
        dk = DeviceBuffer(F * Hp * Wp * 3)
        enc = lambda: M.encode_device(din, F, H, W, Q, 0, out=dk, stream=s, block_size=B)  # noqa: E731
        dec = lambda: M.decode_device(dk, F, H, W, Q, 0, out=drgb, stream=s, block_size=B)  # noqa: E731
        hbm = F * (H * W * 3 + Hp * Wp * 3)
        fma = F * Hp * Wp * 3 * 2 * 2 * B
        for name, fn in (("encode", enc), ("decode", dec)):
            med, lo, hi = timed(fn, s, n, rounds)
            res["cases"].append(dict(
                kernel=f"mdct_{name}", B=B, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                hbm_bytes=hbm, hbm_roofline_fraction=round(hbm / HBM_BYTES_PER_S / (med * 1e-3), 4),
                fp64_fma=fma, fp64_issue_fraction=round(fma / FP64_FMA_PER_S / (med * 1e-3), 4),
                gpixel_per_s=round(F * H * W / (med * 1e-3) / 1e9, 2)))
            print(json.dumps(res["cases"][-1]), flush=True)
        dk.free()
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

"""Time the 2D-LBT kernels: 64 4K frames per launch, B = 8, Q = 32, 1000 epochs.
HIP events on the launch stream around N launches (default 10; the training 2)
after a settling run past the clock ramp; median of R rounds.  Moments,
training, encode and decode are timed separately, each frame with its own
model.

Printed per case: ms per launch and its roofline fraction.  Moments, encode
and decode against HBM (the bytes the algorithm needs: the u8 RGB frame, plus
the u8 coefficient frame for encode and decode, over the measured 6.3 TB/s copy
rate); the training against the float32 MFMA rate: six 64 x 64 x 64 products
per epoch and frame, one workgroup (one CU) per frame, so the roofline of a
launch is that of the CUs it occupies: 64 flop per clock and SIMD, 4 SIMDs, at
the 2.4 GHz of the public specification.

python scripts/bench_lbt.py [N] [R] [--out profiles/lbt_bench.json]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from vcf_amd import synthetic
import vcf_amd.lbt as L
from vcf_amd._lib import call
from vcf_amd.device import DeviceBuffer, Event, Stream, _h, set_device

HBM_BYTES_PER_S = 6.3e12                 # measured copy rate (8.0 TB/s specified)
MFMA_F32_FMA_PER_S_PER_CU = 4 * 32 * 2.4e9   # 64 flop = 32 multiply-adds per clock and SIMD


def timed(fn, s, n, rounds, settle_s=1.0):
    t0 = time.time()
    while time.time() - t0 < settle_s:   # past the clock ramp
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
    n = int(argv[0]) if len(argv) > 0 else 10
    rounds = int(argv[1]) if len(argv) > 1 else 3
    out_fn = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    set_device(0)
    H, W, F, Q, B, epochs = 2160, 3840, 64, 32, 8, L.EPOCHS
    D = B * B
    base = np.stack([synthetic.synth_frame(H, W, s) for s in range(4)])
    frames = np.concatenate([base] * (F // 4))
    din = DeviceBuffer.from_array(frames)
    drgb = DeviceBuffer(F * H * W * 3)
    Hp, Wp = L.padded_shape(H, W, B)[:2]
    n_rows = L.rows(H, W, B)
    s = Stream()
    res = dict(frames=F, H=H, W=W, Q=Q, B=B, epochs=epochs, launches=n, rounds=rounds, cases=[])
    we0, wd0 = L.initial_weights(B)
    init_e = DeviceBuffer.from_array(np.ascontiguousarray(np.broadcast_to(we0, (F, D, D))))
    init_d = DeviceBuffer.from_array(np.ascontiguousarray(np.broadcast_to(wd0, (F, D, D))))
    dwe, dwd = DeviceBuffer(F * D * D * 4), DeviceBuffer(F * D * D * 4)
    d1, d2 = DeviceBuffer(F * D * 8), DeviceBuffer(F * D * D * 8)
    dmean, dloss = DeviceBuffer(F * 4), DeviceBuffer(F * 12)
    dk = DeviceBuffer(F * Hp * Wp * 3)

    def train():
        call("vcf_memcpy_dtod", dwe.ptr, init_e.ptr, F * D * D * 4, _h(s))
        call("vcf_memcpy_dtod", dwd.ptr, init_d.ptr, F * D * D * 4, _h(s))
        L.train_device(d1, d2, F, B, n_rows, dwe, dwd, epochs, mean=dmean, loss=dloss, stream=s)

    mom = lambda: L.moments_device(din, F, H, W, B, d1, d2, stream=s)  # noqa: E731
    enc = lambda: L.encode_device(din, F, H, W, dwe, dmean, Q, 0, out=dk, stream=s, block_size=B)  # noqa: E731
    dec = lambda: L.decode_device(dk, F, H, W, dwd, dmean, Q, 0, out=drgb, stream=s, block_size=B)  # noqa: E731
    coef = F * Hp * Wp * 3
    for name, fn, hbm, reps in (("moments", mom, F * H * W * 3, n), ("train", train, 0, max(1, n // 5)),
                                ("encode", enc, F * H * W * 3 + coef, n), ("decode", dec, F * H * W * 3 + coef, n)):
        med, lo, hi = timed(fn, s, reps, rounds)
        case = {"kernel": f"lbt_{name}", "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
        if name == "train":
            fma = 6 * 64 ** 3 * epochs     # per frame = per CU
            case.update(us_per_epoch=round(med * 1e3 / epochs, 4), multiply_adds_per_frame=fma,
                        mfma_f32_issue_fraction=round(fma / MFMA_F32_FMA_PER_S_PER_CU / (med * 1e-3), 4))
        else:
            case.update(hbm_bytes=hbm, hbm_roofline_fraction=round(hbm / HBM_BYTES_PER_S / (med * 1e-3), 4),
                        gpixel_per_s=round(F * H * W / (med * 1e-3) / 1e9, 2))
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    loss = dloss.download(np.empty((F, 3), np.float32))
    res["final_loss_first_frames"] = [float(x) for x in loss[:4, 0]]
    if out_fn:
        os.makedirs(os.path.dirname(os.path.abspath(out_fn)), exist_ok=True)
        with open(out_fn, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

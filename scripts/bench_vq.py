"""Time the vector quantizer on one 4K frame: `-b 4 -q 256` (VQ.py's defaults:
N = 518 400 vectors of D = 48, K = 256) and `-b 1 -q 32` (color-VQ.py's: N =
8 294 400 pixels of D = 3, K = 32).

Assign and decode are timed with HIP events on the launch stream around N
launches (default 20) after a settling run past the clock ramp, median of R
rounds.  Printed for assign: ms per launch; the float64 issue fraction, three
vector instructions (subtract, multiply, add) per (vector, centroid, element)
against the issue rate behind the 78.6 TFLOP/s FP64 vector peak of the
MI355X's public specification (one instruction per multiply-add: 39.3e12/s);
and the HBM roofline fraction (the frame read once, the labels written, over
the measured 6.3 TB/s copy rate).  The k-means++ init and the whole fit (init
included, seed 0, sklearn's max_iter = 300 and tol = 1e-4) are host-driven
loops that synchronise: wall time of one call each, with the fit's iteration
count, stop reason and inertia.

python scripts/bench_vq.py [N] [R] [--out profiles/vq_bench.json]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from vcf_amd import synthetic
from vcf_amd import vq as VQ
from vcf_amd.device import DeviceBuffer, Event, Stream, set_device

HBM_BYTES_PER_S = 6.3e12         # measured copy rate (8.0 TB/s specified)
FP64_ISSUE_PER_S = 78.6e12 / 2   # FP64 vector instructions per second behind the specified peak


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
    H, W, C = 2160, 3840, 3
    frame = synthetic.synth_frame(H, W, 0)
    dimg = DeviceBuffer.from_array(frame)
    dout = DeviceBuffer(frame.nbytes)
    s = Stream()
    res = dict(H=H, W=W, launches=n, rounds=rounds, cases=[])

    def emit(**row):
        res["cases"].append(row)
        print(json.dumps(row), flush=True)

    for BS, K in ((4, 256), (1, 32)):
        N, D = VQ.shape_of(H, W, C, BS)
        dc, dl = DeviceBuffer(K * D * 8), DeviceBuffer(N * 2)
        ds, dn = DeviceBuffer(K * D * 8), DeviceBuffer(K * 8)
        t0 = time.perf_counter()
        VQ.init_pp_device(dimg, H, W, C, BS, K, 0, dc, stream=s)
        emit(step="init_pp", BS=BS, K=K, N=N, D=D, ms=round((time.perf_counter() - t0) * 1e3, 2))
        t0 = time.perf_counter()
        rep = VQ.fit_device(dimg, H, W, C, BS, K, dc, dl, seed=0, stream=s)
        fit_ms = (time.perf_counter() - t0) * 1e3
        emit(step="fit (init included)", BS=BS, K=K, N=N, D=D, ms=round(fit_ms, 2), n_iter=rep.n_iter,
             stop_reason=rep.stop_reason, relocations=rep.relocations, inertia=rep.inertia,
             ms_per_iteration=round(fit_ms / max(rep.n_iter, 1), 3))
        med, lo, hi = timed(lambda: VQ.assign_device(dimg, H, W, C, BS, dc, K, dl, stream=s), s, n, rounds)
        instr, hbm = 3 * N * K * D, H * W * C + N * 2
        emit(kernel="vq_assign", BS=BS, K=K, N=N, D=D, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
             fp64_instructions=instr, fp64_issue_fraction=round(instr / FP64_ISSUE_PER_S / (med * 1e-3), 4),
             hbm_bytes=hbm, hbm_roofline_fraction=round(hbm / HBM_BYTES_PER_S / (med * 1e-3), 4))
        med, lo, hi = timed(lambda: VQ.accumulate_device(dimg, H, W, C, BS, dl, K, ds, dn, stream=s), s, n, rounds)
        emit(kernel="vq_accumulate", BS=BS, K=K, N=N, D=D, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
             hbm_bytes=hbm, hbm_roofline_fraction=round(hbm / HBM_BYTES_PER_S / (med * 1e-3), 4))
        bad = DeviceBuffer(4)
        bad.fill(0, s)

        def dec():
            from vcf_amd._lib import call
            call("vcf_vq_decode", dl.ptr, H // BS, W // BS, C, BS, dc.ptr, K, dout.ptr, bad.ptr, s.handle)

        med, lo, hi = timed(dec, s, n, rounds)
        emit(kernel="vq_decode", BS=BS, K=K, N=N, D=D, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
             hbm_bytes=hbm, hbm_roofline_fraction=round(hbm / HBM_BYTES_PER_S / (med * 1e-3), 4))
        for b in (dc, dl, ds, dn, bad):
            b.free()
    if out_fn:
        os.makedirs(os.path.dirname(os.path.abspath(out_fn)), exist_ok=True)
        with open(out_fn, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

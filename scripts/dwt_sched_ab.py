"""ABBA of one field of the 2D-DWT kernel schedule (vcf_dwt_schedule,
include/vcf_amd_ab.h) against the library's default on config C3 (8 4K frames,
l=5, bior4.4, Q=32):

  python scripts/dwt_sched_ab.py FIELD encode|decode [--lifting] [-n N] [-r R] VALUE...

e.g. `dec21_brows decode 60 90 108`, `enc_bands encode 1 2 4 8`, `band21 decode 0`,
`lift_fused encode --lifting 0`.  Every setting runs the A/B library's twins of
the product entries (vcf_dwt_dz_*_sched; "default" = a NULL schedule), interleaved
over R rounds of N launches in alternating order, timed with HIP events on the
launch stream.  Prints one JSON line: median ms per launch and an output
checksum per setting (a schedule never changes a byte)."""
import argparse
import ctypes
import json
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import vcf_amd._lib as L
import vcf_amd.dwt as DW
from vcf_amd.device import DeviceBuffer, Event, Stream, set_device
from vcf_amd.synthetic import synth_frame

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("field", choices=sorted(L.DwtSchedule.DEFAULTS))
ap.add_argument("what", choices=["encode", "decode"])
ap.add_argument("values", nargs="+", type=int)
ap.add_argument("--lifting", action="store_true")
ap.add_argument("-n", type=int, default=40, help="launches per timed round")
ap.add_argument("-r", type=int, default=6, help="rounds")
a = ap.parse_args()

set_device(0)
H, W, F, LV, Q = 2160, 3840, 8, 5, 32
w = DW.wavelet_index(os.environ.get("WAVELET", "bior4.4"))
_, pb, wb = DW.layout(H, W, LV)
frames = np.stack([synth_frame(H, W, s) for s in range(F)])
din, dws, dpk = DeviceBuffer.from_array(frames), DeviceBuffer(F * wb), DeviceBuffer(F * pb)
dout = DeviceBuffer(F * H * W * 3)
s = Stream()
lift = "_lift" if a.lifting else ""
settings = {"default": None, **{str(v): ctypes.byref(L.DwtSchedule(**{a.field: v})) for v in a.values}}


def run(sched, what=a.what):
    if what == "encode":
        L.call_ab(f"vcf_dwt_dz_encode{lift}_sched", sched, din.ptr, F, H, W, w, LV, Q, dpk.ptr, dws.ptr, s.handle)
    else:
        L.call_ab(f"vcf_dwt_dz_decode{lift}_sched", sched, dpk.ptr, F, H, W, w, LV, Q, dout.ptr, dws.ptr, s.handle)


run(None, "encode")   # the decode's input
res, crc = {k: [] for k in settings}, {}
out = dpk if a.what == "encode" else dout
for k, sched in settings.items():
    for _ in range(20):
        run(sched)
    s.synchronize()
    crc[k] = zlib.crc32(out.download(np.empty(out.nbytes, np.uint8)).tobytes())
order = list(settings)
for r in range(a.r):
    for k in (order if r % 2 == 0 else order[::-1]):
        e0, e1 = Event(), Event()
        e0.record(s)
        for _ in range(a.n):
            run(settings[k])
        e1.record(s)
        s.synchronize()
        res[k].append(e0.elapsed_ms(e1) / a.n)
print(json.dumps({"what": f"C3 {a.what}{' (lifting)' if a.lifting else ''} ms per 8 x 4K by {a.field} "
                          "(vcf_dwt_schedule; default = the library's rule)",
                  "same_bytes": len(set(crc.values())) == 1, "crc": crc,
                  "ms_median": {k: round(float(np.median(v)), 4) for k, v in res.items()}}), flush=True)
